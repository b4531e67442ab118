// rnde_node_tile.h -- TrackedNeuralODE over a Dense chain on the tile layout of rnde_ffjordt.h (rnde_node_create_tiled, engine 4): the
// right-hand side is the chain itself, f(u, t) = y_n, with no trace row and no probe.  What TrackedFFJORD's chain dynamics built serves here
// unchanged: the geometry (FcGeo, fc_geo), the parameter load (FcDyn::load_params), the chain evaluation (fc_chain), the layer products
// (ft_fwd / ft_tr), the meeting (tile_meet over rnde_meet.h) and the controller (advance_state_t over R = D rows).  The Runge-Kutta loop
// of rnde_ffjord_tile.h is restated for a state of D rows; the reverse sweep is rnde_bnode_tile.h.
//
// Layout: one workgroup of four waves per 16 batch columns (a tile).  The padded weights stay resident in LDS (Wl[in][outp + 1], the t
// column and the bias as per-output vectors beside them); activations are [feature][16]; every layer's output stays in LDS (the reverse
// reads the activation derivatives from it) and two vectors carry the VJP down the chain.  The state is [D][Bp] in global memory, each tile
// touching its own 16 columns: D is limited by LDS bytes (the input tile [DP][16]), not by a row count.
//
//     LDS floats = align4(weights) + DP * 16 (input) + sum_l outp_l * 16 (outputs) + 2 * MP * 16 (VJP vectors) + 128 (reductions, meeting)
//
// The solve and the reverse kernel use the same view, so one byte count (NtDyn::lds_floats) is the limit of both: at most 160 KB.
//
// Forward solve: the whole adaptive Tsit5 solve in one launch, as rnde_ffjord_tile_solve_kernel: once per attempt every tile forms its
// partial of the error norm and the tiles meet; partials are summed in tile order in double, so every tile runs the same controller on the
// same bits and a solve is bit-identical run to run (empty tiles of a larger max_batch never exist: the grid is the batch's tiles).  A
// meeting that times out raises the abort word and ends the launch; the host reports it by name.
#pragma once
#include "rnde_tile_meet.h"        // tile_meet; rnde_ffjordt.h, rnde_meet.h
#include "rnde_ffjordc.h"          // FcGeo, fc_geo, FcDyn::load_params, fc_chain
#include "rnde_track_rec.h"        // FfAttRec; the initial-step rule's scalar reverse
#include "rnde_save_plan.h"        // SaveRange

namespace rnde {

struct NtLds {
    float* W;
    float* X;                          // [DP][16]: the chain's input (padded rows zero)
    float* Y;                          // every layer's output, layer l at Y + yoff[l] ([outp_l][16], padded rows zero)
    float *V0, *V1;                    // [MP][16]: v_l going down the chain (reverse sweep)
    float* red;                        // 128 floats (the meeting keeps doubles at red + 64)
};

struct NtDyn {
    __host__ __device__ static int lds_floats(const FcGeo& G) { return ft_align4(G.wfloats) + G.DP * 16 + G.yfloats + 2 * G.MP * 16 + 128; }
    // the reverse sweep's per-tile global workspace: stage inputs, stage values, stage cotangents (7 each), ub, ub-next, yb
    __host__ __device__ static size_t rev_ws_floats(const FcGeo& G) { return (size_t)24 * G.D * 16; }
    __device__ static NtLds lds(const FcGeo& G, float* smem) {
        NtLds L;
        L.W = smem;
        float* b = smem + ft_align4(G.wfloats);      // (an even number of floats up to red: the meeting's doubles are 8-byte aligned)
        L.X = b; b += G.DP * 16;
        L.Y = b; b += G.yfloats;
        L.V0 = b; b += G.MP * 16; L.V1 = b; b += G.MP * 16;
        L.red = b;
        return L;
    }
    // kout[o * ks + c] = f_o(X, t) for o < D.  Opens with the barrier ahead of the first read of L.X (and of the parameters), ends behind one.
    __device__ static __forceinline__ void eval(const FcGeo& G, const NtLds& L, float t, float* kout, int ks, int tid) {
        __syncthreads();
        fc_chain(G, L.W, L.X, L.Y, t, tid >> 6, tid & 63, [&](int o, int cc, float f) { kout[(size_t)o * ks + cc] = f; });
    }
};

struct NodeTileSolveParams {
    StepParams F;                    // the controller's view (F.D = D rows; F.ctl / meta / ctl_final: tile 0's)
    FcGeo G;
    const float* p;
    const float* x;                  // D x B caller layout
    float* ws;                       // [10][D][Bp]: uprev, unew, (unused), k1..k7
    float* tape;                     // [max_attempts + 1][D][Bp] or NULL
    float* u_out;                    // D x B caller layout or NULL
    float* norm;                     // [ntiles][8] + 512: each tile's initial-step norms
    InitRec* initrec_t;              // [ntiles]
    StepState* ctl_t;                // [ntiles]: where tiles other than 0 write the state before attempt 0
    Meet meet;                       // three rows per meeting
    unsigned* xcc;                   // [ntiles] (one-XCD meeting: the host checks they agree)
    int xcd_slot;
    int Bp;
};

struct NtStepRec { float t, dt, eest, svb; };     // one accepted step, in forward order; svb = cotangent of its saved value EEst * dt (as FfStepRec)

struct NodeTileRevParams {
    FcGeo G;
    const float* p;
    const float* tape;                // [n_acc + 1][D][Bp]
    const NtStepRec* rec;             // [n_acc]
    const float* u_bar;               // D x B caller layout
    float* ws;                        // [ntiles][NtDyn::rev_ws_floats]
    float* pacc;                      // [ntiles][P]
    float* x_bar;                     // D x B caller layout (may be NULL)
    int n_acc, B, Bp;
    float reltol, abstol;
    // the tracked sweep (rnde_node_tile_reverse_kernel<true>) alone
    const FfAttRec* att;              // [n_att]
    int n_att, track_initdt;
    InitRec init;                     // the taped solve's initial-step record
    float t0;
    double* tspan_out;                // [2]: (t0-bar, t1-bar), written by tile 0
    Meet meet;                        // three rows per meeting: one per attempt, then two for the initial step
    unsigned* xcc;                    // [ntiles] (one-XCD meeting: the host checks they agree)
    int xcd_slot;
    // a saving tape (rnde_node_tile_reverse_kernel<*, true>) alone: u_bar is then D x nsave x B, the cotangents of the saved states
    const float* sv_t;                // [nsave]: the tape's own copy of the save times
    const SaveRange* rng;             // the save indices of record n of the sweep's walk: [n_att] by attempt (tracked), [n_acc] by accepted step
    int nsave, save_t0;               // save_t0: index 0 is the start (sv_t[0] == t0), its cotangent goes straight to x_bar
};

// The whole adaptive solve in one launch (also the replay along F.replay).
// SAVE (a handle with a saveat capacity, F.nsave > 0): behind the controller of an accepted attempt every tile writes u(ts) for the save
// indices [S.next_save, Sn.next_save) of the step -- unew itself at the step's end, uprev + dt sum_j b_j(theta) k_j inside it (the Tsit5
// dense output, dense_weights; the arithmetic of chain_dense_points) -- into F.sv_out (D x nsave x B, caller layout).  Every tile holds
// the same controller bits, so the range is uniform: no meeting and no barrier beyond the loop's.  The save times never enter the
// controller: a saving solve takes the end-state solve's attempts bit for bit.  Without SAVE the kernel is the end-state solve unchanged.
template <bool SAVE = false>
__global__ __launch_bounds__(kFtThreads) void rnde_node_tile_solve_kernel(const NodeTileSolveParams Q) {
    extern __shared__ float nt_smem[];
    if (!Q.meet.global && (int)(blockIdx.x & 7) != Q.xcd_slot) return;
    const int tile = Q.meet.global ? (int)blockIdx.x : (int)(blockIdx.x >> 3);
    const int tid = threadIdx.x, lane = tid & 63;
    const FcGeo& G = Q.G;
    const int D = G.D, Bp = Q.Bp, B = Q.F.B, col0 = tile * 16;
    if (!Q.meet.global && tid == 0) Q.xcc[tile] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15;
    StepParams P = Q.F;
    P.initpart = Q.norm + 8 * tile;
    P.initrec = Q.initrec_t + tile;
    const bool lead = tile == 0 && tid == 0;
    const NtLds L = NtDyn::lds(G, nt_smem);
    FcDyn::load_params(G, Q.p, L.W, tid);
    const size_t RB = (size_t)D * Bp;
    float* U = Q.ws + col0;
    float* UN = Q.ws + RB + col0;
    auto K = [&](int s) { return Q.ws + (size_t)(3 + s) * RB + col0; };
    const float rt = P.reltol, at = P.abstol;
    const double N = (double)D * (double)B;
    const int nel = D * 16;

    // ---- initial state, f(u0), the initial-step rule (the arithmetic of rnde_ffjord_tile_solve_kernel over D rows) ----
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {     // (rows >= D of L.X stay zero for the whole solve)
        const int r = idx >> 4, c = idx & 15, col = col0 + c;
        const float v = (r < D && col < B) ? Q.x[(size_t)col * D + r] : 0.f;
        if (r < D) U[(size_t)r * Bp + c] = v;
        L.X[idx] = v;
    }
    NtDyn::eval(G, L, P.t0 + 0.f, K(0), Bp, tid);
    float pa = 0.f, pb = 0.f;
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        if (col0 + c >= B) continue;
        const size_t ix = (size_t)r * Bp + c;
        const float xv = U[ix], kv = K(0)[ix], sk = at + fabsf(xv) * rt;
        const float a = xv / sk, b = kv / sk;
        pa += a * a; pb += b * b;
    }
    double sm[3];
    if (!tile_meet(Q.meet, L.red, 0, pa, pb, 0.f, sm, tile, tid)) return;
    float dt0;
    {
        const float d0 = (float)sqrt(sm[0] / N), d1 = (float)sqrt(sm[1] / N), dtmax = P.t1 - P.t0;
        int c0 = 0, cl = 0;
        if (d0 < 1e-5f || d1 < 1e-5f) { dt0 = 1e-6f; c0 = 1; }
        else dt0 = (d0 / d1) / 100.f;
        if (dtmax < dt0) { dt0 = dtmax; cl = 1; }
        if (tid == 0) { P.initrec->d0 = d0; P.initrec->d1 = d1; P.initrec->dt0 = dt0; P.initrec->dt0_const = c0; P.initrec->dt0_clamped = cl; }
    }
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        const size_t ix = (size_t)r * Bp + c;
        L.X[idx] = U[ix] + dt0 * K(0)[ix];
    }
    NtDyn::eval(G, L, P.t0 + dt0, K(1), Bp, tid);
    float pc = 0.f;
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        if (col0 + c >= B) continue;
        const size_t ix = (size_t)r * Bp + c;
        const float sk = at + fabsf(U[ix]) * rt;
        const float a = (K(1)[ix] - K(0)[ix]) / sk;
        pc += a * a;
    }
    if (!tile_meet(Q.meet, L.red, 1, pc, 0.f, 0.f, sm, tile, tid)) return;
    if (tid == 0) P.initpart[2] = (float)sm[0];       // advance_state reads the third initial norm as a one-entry partial
    __syncthreads();
    __threadfence_block();
    StepState S = advance_state(P, 0, lane, tid == 0, tile == 0 ? &P.ctl[0] : Q.ctl_t + tile);
    int n_acc = 0;
    if constexpr (SAVE) {
        if (S.next_save > 0)                                   // save_start: sv_t[0] == t0, index 0 is x itself
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                if (col0 + c < B) P.sv_out[((size_t)(col0 + c) * P.nsave) * D + r] = U[(size_t)r * Bp + c];
            }
    }
    for (int n = 0; !S.done; ++n) {
        const float t = S.t;
        const float dt = (P.t1 - S.t < S.dtp) ? (P.t1 - S.t) : S.dtp;
        for (int s = 1; s < 7; ++s) {                      // stage s + 1: input uprev + dt sum_j a_{s+1, j} k_j
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                const size_t ix = (size_t)r * Bp + c;
                float acc = 0.f;
                for (int j = 0; j < s; ++j) acc = fmaf(tsA_rt(s, j), K(j)[ix], acc);
                const float g = U[ix] + dt * acc;
                L.X[idx] = g;
                if (s == 6) UN[ix] = g;
            }
            NtDyn::eval(G, L, t + kTsC[s] * dt, K(s), Bp, tid);
        }
        float part = 0.f;
        for (int idx = tid; idx < nel; idx += kFtThreads) {   // embedded error estimate, SURVEY.md B.3
            const int r = idx >> 4, c = idx & 15;
            if (col0 + c >= B) continue;
            const size_t ix = (size_t)r * Bp + c;
            float E = 0.f;
            for (int j = 0; j < 7; ++j) E += kTsBt[j] * K(j)[ix];
            const float ut = dt * E, sk = at + fmaxf(fabsf(U[ix]), fabsf(UN[ix])) * rt, rr = ut / sk;
            part += rr * rr;
        }
        double xs[3];
        if (!tile_meet(Q.meet, L.red, 2 + n, part, 0.f, 0.f, xs, tile, tid)) return;
        const float none[4] = {0.f, 0.f, 0.f, 0.f};
        const StepState Sn = advance_state_t<true>(P, n + 1, lane, lead, &P.ctl[(n + 1) & 1], none, S, xs);
        if constexpr (SAVE) {
            for (int si = S.next_save; si < Sn.next_save; ++si) {      // (a rejected attempt leaves next_save alone: an empty range)
                const float ts = P.sv_t[si];
                const bool at_end = ts == Sn.t;
                float bw[7];
                dense_weights((ts - t) / dt, bw);
                for (int idx = tid; idx < nel; idx += kFtThreads) {
                    const int r = idx >> 4, c = idx & 15;
                    if (col0 + c >= B) continue;
                    const size_t ix = (size_t)r * Bp + c;
                    float o = UN[ix];
                    if (!at_end) {
                        float acc = bw[0] * K(0)[ix];
#pragma unroll
                        for (int j = 1; j < 7; ++j) acc += bw[j] * K(j)[ix];      // (unrolled: bw stays in registers)
                        o = U[ix] + dt * acc;
                    }
                    P.sv_out[((size_t)(col0 + c) * P.nsave + si) * D + r] = o;
                }
            }
        }
        if (Sn.n_acc > S.n_acc) {                          // accepted: tape uprev, then unew -> uprev, k7 -> k1
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                const size_t ix = (size_t)r * Bp + c;
                if (Q.tape) Q.tape[(size_t)n_acc * RB + col0 + ix] = U[ix];
                U[ix] = UN[ix];
                K(0)[ix] = K(6)[ix];
            }
            ++n_acc;
        }
        S = Sn;
    }
    if (lead) *P.ctl_final = S;
    __syncthreads();
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        const size_t ix = (size_t)r * Bp + c;
        if (Q.tape) Q.tape[(size_t)n_acc * RB + col0 + ix] = U[ix];
        if (col0 + c < B && Q.u_out) Q.u_out[(size_t)(col0 + c) * D + r] = U[ix];
    }
}

// out = f(u, p, t), D x B caller layout (the parity instrument).  One workgroup per tile; ws: [ntiles][D][16].
__global__ __launch_bounds__(kFtThreads) void rnde_node_tile_feval_kernel(const FcGeo G, const float* __restrict__ p, const float* __restrict__ x, float t,
                                                                         int B, float* __restrict__ ws, float* __restrict__ out) {
    extern __shared__ float nt_smem[];
    const int tile = blockIdx.x, tid = threadIdx.x, D = G.D, col0 = tile * 16;
    const NtLds L = NtDyn::lds(G, nt_smem);
    FcDyn::load_params(G, p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        L.X[idx] = (r < D && col < B) ? x[(size_t)col * D + r] : 0.f;
    }
    float* k = ws + (size_t)tile * D * 16;
    NtDyn::eval(G, L, t, k, 16, tid);
    for (int idx = tid; idx < D * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        if (col < B) out[(size_t)col * D + r] = k[idx];
    }
}

}  // namespace rnde
