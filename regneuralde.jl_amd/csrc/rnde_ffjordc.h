// rnde_ffjordc.h -- TrackedFFJORD's default dynamics (ffjord.jl:21-27: Tracker.forward(z -> m(z, t), z) and back(e)) for a chain of Dense
// layers, plain (Chain) or time dependent (TDChain: t appended to every layer's input), on the tiled layout of rnde_ffjordt.h
// (rnde_ffjord_create_chain, engine 2).
//
// Dynamics, y_0 = z:   a_l = W_l y_{l-1} + wt_l t + b_l,   y_l = phi_l(a_l),   f = y_n,   d_l = phi_l' taken from y_l (act_dy)
//     v_n = d_n .* e,   m_l = W_{l+1}' v_{l+1} (the z columns only),   v_l = d_l .* m_l,   eJ = W_1' v_1,   F = [f; -e . eJ]
// KIN: F = [f; -e . eJ; sum f^2; sum eJ^2] (ffjord.jl:53-66).  The exact trace (sample, feval exact) is D passes of the same VJP with
// unit probes, as the reference's jacobian_fn.
//
// Geometry: rnde_ffjordt.h's.  One workgroup of four waves per 16 batch columns; the padded weights resident in LDS as Wl[in][ld]
// (ld = outp + 1), the t column and the bias as two per-output vectors beside them (the t column is an epilogue term, `in` is not padded
// to in + 1); activations [feature][16]; layer products through ft_fwd / ft_tr.  Every layer's output stays in LDS for the VJP (d_l is read
// from it), two more vectors carry v_l down the chain.  Limits come from bytes: fc_lds_floats(G) * 4 <= 160 KB, checked at create.
#pragma once
#include "rnde_ffjordt.h"

namespace rnde {

constexpr int kFcMaxLayers = 8;        // RNDE_MAX_LAYERS
constexpr int kFcMaxW = 64;            // no layer output, no layer input (its time row apart) and no state above 64 rows

struct FcGeo {
    int n, D, P, td, DP, MP;           // layers, data rows, parameters, time_dep, padded D, the widest padded layer
    int dims[kFcMaxLayers + 1], act[kFcMaxLayers];
    int off[kFcMaxLayers];             // parameter offset of each layer: W (in x out as stored: p[i * out + o]), then the t row, then b
    int inp[kFcMaxLayers], outp[kFcMaxLayers], ld[kFcMaxLayers];
    int woff[kFcMaxLayers], voff[kFcMaxLayers];      // LDS offsets (floats) of Wl and of the two vectors wt, b (outp each)
    int yoff[kFcMaxLayers];            // offset of layer l's output inside the Y block
    int wfloats, yfloats;
};

__host__ inline FcGeo fc_geo(int n, const int* dims, const int* act, int td) {
    FcGeo G{};
    G.n = n; G.D = dims[0]; G.td = td ? 1 : 0; G.DP = ft_pad16(dims[0]); G.MP = G.DP;
    int o = 0, w = 0, y = 0;
    for (int l = 0; l <= n; ++l) G.dims[l] = dims[l];
    for (int l = 0; l < n; ++l) {
        G.act[l] = act[l];
        G.off[l] = o; o += (dims[l] + G.td) * dims[l + 1] + dims[l + 1];
        G.inp[l] = ft_pad16(dims[l]); G.outp[l] = ft_pad16(dims[l + 1]); G.ld[l] = G.outp[l] + 1;
        G.woff[l] = w; w += G.inp[l] * G.ld[l];
        G.yoff[l] = y; y += G.outp[l] * 16;
        if (G.outp[l] > G.MP) G.MP = G.outp[l];
    }
    for (int l = 0; l < n; ++l) { G.voff[l] = w; w += 2 * G.outp[l]; }
    G.P = o; G.wfloats = w; G.yfloats = y;
    return G;
}
// LDS floats of the solve / feval / reverse kernels: parameters, X, E, every layer's output, two VJP vectors, reduction scratch
__host__ __device__ inline int fc_lds_floats(const FcGeo& G) { return ft_align4(G.wfloats) + 2 * G.DP * 16 + G.yfloats + 2 * G.MP * 16 + 128; }

struct FcLds {
    float* W;
    float *X, *E;                      // [DP][16]: the chain's input, the probe
    float* Y;                          // every layer's output, layer l at Y + yoff[l] ([outp_l][16], padded rows zero)
    float *V0, *V1;                    // [MP][16]: v_l going down the chain
    float* red;                        // 128 floats (the meeting keeps doubles at red + 64)
};
__device__ inline FcLds fc_lds(const FcGeo& G, float* smem) {
    FcLds L;
    L.W = smem;
    float* b = smem + ft_align4(G.wfloats);
    L.X = b; b += G.DP * 16; L.E = b; b += G.DP * 16;
    L.Y = b; b += G.yfloats;
    L.V0 = b; b += G.MP * 16; L.V1 = b; b += G.MP * 16;
    L.red = b;
    return L;
}

// parameters into LDS, zero-padded (every thread of the workgroup)
__device__ inline void fc_load_params(const FcGeo& G, const float* __restrict__ p, float* W, int tid) {
    for (int l = 0; l < G.n; ++l) {
        const int ld = G.ld[l], in = G.dims[l], out = G.dims[l + 1], n = G.inp[l] * ld, op = G.outp[l];
        float* w = W + G.woff[l];
        for (int idx = tid; idx < n; idx += kFtThreads) {
            const int i = idx / ld, o = idx - i * ld;
            w[idx] = (i < in && o < out) ? p[G.off[l] + i * out + o] : 0.f;
        }
        float* v = W + G.voff[l];
        for (int idx = tid; idx < 2 * op; idx += kFtThreads) {
            const int k = idx / op, o = idx - k * op;
            float x = 0.f;
            if (o < out) x = k == 0 ? (G.td ? p[G.off[l] + in * out + o] : 0.f) : p[G.off[l] + (in + G.td) * out + o];
            v[idx] = x;
        }
    }
}

// y_l = phi_l(W_l y_{l-1} + wt_l t + b_l) for every layer: X -> Y.  last(o, c, y): called for the rows o < D of the last layer.
template <class Last>
__device__ __forceinline__ void fc_chain(const FcGeo& G, const float* W, const float* X, float* Y, float t, int wave, int lane, Last&& last) {
    const int c = lane & 15;
    for (int l = 0; l < G.n; ++l) {
        const float *wt = W + G.voff[l], *b = wt + G.outp[l];
        const int out = G.dims[l + 1], code = G.act[l];
        float* y = Y + G.yoff[l];
        const bool fin = l == G.n - 1;
        ft_fwd(W + G.woff[l], G.ld[l], G.inp[l], G.outp[l], l ? Y + G.yoff[l - 1] : X, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = r0 + j;
                float a = 0.f;
                if (o < out) { a = act_fwd(code, fmaf(wt[o], t, v[j] + b[o])); if (fin) last(o, c, a); }
                y[o * 16 + c] = a;
            }
        });
        __syncthreads();
    }
}

// eJ = W_1' v_1 from v_n in Va ([outp_n][16]); epi(r0, v) sees the rows of eJ.  Va / Vb alternate; ends without a barrier.
template <class Epi>
__device__ __forceinline__ void fc_pull(const FcGeo& G, const float* W, const float* Y, float* Va, float* Vb, int wave, int lane, Epi&& epi) {
    const int c = lane & 15;
    for (int l = G.n - 1; l >= 1; --l) {       // m_{l-1} = W_l' v_l, v_{l-1} = d_{l-1} .* m_{l-1}
        const float* y = Y + G.yoff[l - 1];
        const int code = G.act[l - 1];
        ft_tr(W + G.woff[l], G.ld[l], G.inp[l], G.outp[l], Va, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; Vb[ix] = v[j] * act_dy(code, y[ix]); }
        });
        __syncthreads();
        float* s = Va; Va = Vb; Vb = s;
    }
    ft_tr(W + G.woff[0], G.ld[0], G.inp[0], G.outp[0], Va, wave, lane, epi);
}

// One evaluation of the augmented right-hand side for the 16 columns of a tile (the contract of ft_eval).
//   pre: L.X holds the data rows of the input ([DP][16], padded rows zero), L.E the probe (Hutchinson; zero columns where not valid).
//   out: kout[r * ks + c] = fsign * f_r (r < D), kout[D * ks + c] = tsign * tr.  exact: D unit-probe passes.
//   KIN (Hutchinson only): kout[(D + 1) * ks + c] = sum f^2, kout[(D + 2) * ks + c] = sum eJ^2.
//   Every thread of the workgroup calls it; it ends behind a barrier.
template <bool KIN = false>
__device__ __forceinline__ void fc_eval(const FcGeo& G, const FcLds& L, float t, float* kout, int ks, int exact, float fsign, float tsign, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, n = G.n;
    float pke = 0.f, pjn = 0.f, part = 0.f;
    fc_chain(G, L.W, L.X, L.Y, t, wave, lane, [&](int o, int cc, float f) { kout[(size_t)o * ks + cc] = fsign * f; });
    const float* yn = L.Y + G.yoff[n - 1];
    const int cn = G.act[n - 1], nv = G.outp[n - 1] * 16;
    if constexpr (KIN)
        for (int idx = tid; idx < nv; idx += kFtThreads) pke = fmaf(yn[idx], yn[idx], pke);      // (idx & 15 = lane & 15; padded rows are zero)
    if (exact) {
        for (int i = 0; i < D; ++i) {
            for (int idx = tid; idx < nv; idx += kFtThreads) L.V0[idx] = (idx >> 4) == i ? act_dy(cn, yn[idx]) : 0.f;
            __syncthreads();
            fc_pull(G, L.W, L.Y, L.V0, L.V1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) part += (r0 + j == i) ? v[j] : 0.f;
            });
            __syncthreads();
        }
    } else {
        for (int idx = tid; idx < nv; idx += kFtThreads) L.V0[idx] = act_dy(cn, yn[idx]) * L.E[idx];      // (rows >= D: the probe is zero)
        __syncthreads();
        fc_pull(G, L.W, L.Y, L.V0, L.V1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                part = fmaf(L.E[(r0 + j) * 16 + c], v[j], part);
                if constexpr (KIN) pjn = fmaf(v[j], v[j], pjn);      // (rows >= D: W_1's padded rows are zero)
            }
        });
    }
    const float tr = ft_colsum(part, L.red, tid);
    if (tid < 16) kout[(size_t)D * ks + tid] = tsign * tr;
    if constexpr (KIN) {
        const float ke = ft_colsum(pke, L.red, tid);
        const float jn = ft_colsum(pjn, L.red, tid);
        if (tid < 16) { kout[(size_t)(D + 1) * ks + tid] = ke; kout[(size_t)(D + 2) * ks + tid] = jn; }
    }
    __syncthreads();
}

struct FcSolveParams {
    StepParams F;                    // the controller's view (F.D = R rows; F.ctl / meta / ctl_final: tile 0's)
    FcGeo G;
    const float* p;
    const float* x;                  // D x B caller layout
    const float* e;                  // D x B caller layout (dir = +1), NULL (dir = -1: exact trace)
    float* ws;                       // [10][R][Bp]: uprev, unew, (unused), k1..k7
    float* tape;                     // [max_attempts + 1][R][Bp] or NULL
    float* logpx;                    // B (dir = +1) or NULL
    float* x_out;                    // D x B caller layout or NULL
    float* norm;                     // [ntiles][8] + 512
    InitRec* initrec_t;              // [ntiles]
    StepState* ctl_t;                // [ntiles]
    MwMeet meet;
    unsigned* xcc;                   // [ntiles] (one-XCD meeting: the host checks they agree)
    int xcd_slot;
    int dir, Bp, ntiles;
    float tbase;                     // dir = -1: t1
    float* reg;                      // kinetic solves: 2 x B; NULL otherwise
};

// ft_meet on a bare MwMeet: publish this tile's three partials, collect everybody's sums in tile order; false when the meeting timed out.
__device__ __forceinline__ bool fc_meet(const MwMeet& M, float* red, int seq, float a, float b, float c, double (&out)[3], int tile, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    a = wave_sum_f(a); b = wave_sum_f(b); c = wave_sum_f(c);
    if (lane == 0) { red[wave] = a; red[4 + wave] = b; red[8 + wave] = c; }
    __syncthreads();
    double* RD = (double*)(red + 64);
    if (wave == 0) {
        const float mine[3] = {((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7], ((red[8] + red[9]) + red[10]) + red[11]};
        double o[3];
        const bool ok = mw_exchange3(M, seq, mine, o, tile, lane);
        if (lane == 0) { RD[0] = o[0]; RD[1] = o[1]; RD[2] = o[2]; red[70] = ok ? 1.f : 0.f; }
    }
    __syncthreads();
    const bool ok = red[70] != 0.f;
    out[0] = RD[0]; out[1] = RD[1]; out[2] = RD[2];
    __syncthreads();
    return ok;
}

// The whole adaptive solve in one launch (the structure of rnde_ffjordt_solve_kernel): forward (dir = +1, Hutchinson), replay along
// P.replay, sampling (dir = -1, exact trace, tau = t1 - t).
template <bool KIN>
__global__ __launch_bounds__(kFtThreads) void rnde_ffjordc_solve_kernel(const FcSolveParams Q) {
    extern __shared__ float ft_smem[];
    if (!Q.meet.global && (int)(blockIdx.x & 7) != Q.xcd_slot) return;
    const int tile = Q.meet.global ? (int)blockIdx.x : (int)(blockIdx.x >> 3);
    const int tid = threadIdx.x, lane = tid & 63;
    const FcGeo& G = Q.G;
    const int D = G.D, R = D + (KIN ? 3 : 1), Bp = Q.Bp, B = Q.F.B, col0 = tile * 16;
    if (!Q.meet.global && tid == 0) Q.xcc[tile] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15;
    StepParams P = Q.F;
    P.initpart = Q.norm + 8 * tile;
    P.initrec = Q.initrec_t + tile;
    const bool lead = tile == 0 && tid == 0;
    const FcLds L = fc_lds(G, ft_smem);
    fc_load_params(G, Q.p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        L.E[idx] = (Q.dir > 0 && r < D && col < B) ? Q.e[(size_t)col * D + r] : 0.f;
        L.X[idx] = 0.f;
    }
    const size_t RB = (size_t)R * Bp;
    float* U = Q.ws + col0;
    float* UN = Q.ws + RB + col0;
    auto K = [&](int s) { return Q.ws + (size_t)(3 + s) * RB + col0; };
    const int exact = Q.dir < 0 ? 1 : 0;
    const float fsign = Q.dir > 0 ? 1.f : -1.f, tsign = Q.dir > 0 ? -1.f : 1.f;
    auto eval = [&](float time, float* kout) { fc_eval<KIN>(G, L, Q.dir > 0 ? time : Q.tbase - time, kout, Bp, exact, fsign, tsign, tid); };
    const float rt = P.reltol, at = P.abstol;
    const double N = (double)R * (double)B;
    const int nel = R * 16;
    __syncthreads();

    // ---- initial state, f(u0), the initial-step rule ----
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15, col = col0 + c;
        const float v = (r < D && col < B) ? Q.x[(size_t)col * D + r] : 0.f;
        U[(size_t)r * Bp + c] = v;
        if (r < D) L.X[r * 16 + c] = v;
    }
    __syncthreads();
    eval(P.t0 + 0.f, K(0));
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
    if (!fc_meet(Q.meet, L.red, 0, pa, pb, 0.f, sm, tile, tid)) return;
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
        if (r < D) L.X[r * 16 + c] = U[ix] + dt0 * K(0)[ix];
    }
    __syncthreads();
    eval(P.t0 + dt0, K(1));
    float pc = 0.f;
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        if (col0 + c >= B) continue;
        const size_t ix = (size_t)r * Bp + c;
        const float sk = at + fabsf(U[ix]) * rt;
        const float a = (K(1)[ix] - K(0)[ix]) / sk;
        pc += a * a;
    }
    if (!fc_meet(Q.meet, L.red, 1, pc, 0.f, 0.f, sm, tile, tid)) return;
    if (tid == 0) P.initpart[2] = (float)sm[0];       // advance_state reads the third initial norm as a one-entry partial
    __syncthreads();
    __threadfence_block();
    StepState S = advance_state(P, 0, lane, tid == 0, tile == 0 ? &P.ctl[0] : Q.ctl_t + tile);
    int n_acc = 0;
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
                if (r < D) L.X[r * 16 + c] = g;
                if (s == 6) UN[ix] = g;
            }
            __syncthreads();
            eval(t + kTsC[s] * dt, K(s));
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
        if (!fc_meet(Q.meet, L.red, 2 + n, part, 0.f, 0.f, xs, tile, tid)) return;
        const float none[4] = {0.f, 0.f, 0.f, 0.f};
        const StepState Sn = advance_state_t<true>(P, n + 1, lane, lead, &P.ctl[(n + 1) & 1], none, S, xs);
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
        if (r < D && col0 + c < B && Q.x_out) Q.x_out[(size_t)(col0 + c) * D + r] = U[ix];
    }
    if (tid < 16 && col0 + tid < B && Q.logpx) {
        float lp = 0.f;
        for (int r = 0; r < D; ++r) {
            const float z = U[(size_t)r * Bp + tid];
            lp += -(1.8378770664093453f + z * z) * 0.5f;
        }
        Q.logpx[col0 + tid] = lp - U[(size_t)D * Bp + tid];
    }
    if constexpr (KIN)
        if (tid < 16 && col0 + tid < B) {
            Q.reg[col0 + tid] = U[(size_t)(D + 1) * Bp + tid];
            Q.reg[(size_t)B + col0 + tid] = U[(size_t)(D + 2) * Bp + tid];
        }
}

// One evaluation of the augmented right-hand side per column (the parity instrument): out (D + 1) x B caller layout, the trace row -e . eJ
// (exact: -tr J).  One workgroup per tile; ws: [ntiles][R][16].  KIN: (D + 3) x B, Hutchinson only.
template <bool KIN>
__global__ __launch_bounds__(kFtThreads) void rnde_ffjordc_feval_kernel(const FcGeo G, const float* __restrict__ p, const float* __restrict__ x,
                                                                       const float* __restrict__ e, float t, int B, int exact, float* __restrict__ ws,
                                                                       float* __restrict__ out) {
    extern __shared__ float ft_smem[];
    const int tile = blockIdx.x, tid = threadIdx.x, D = G.D, R = D + (KIN ? 3 : 1), col0 = tile * 16;
    const FcLds L = fc_lds(G, ft_smem);
    fc_load_params(G, p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        const bool ok = r < D && col < B;
        L.X[idx] = ok ? x[(size_t)col * D + r] : 0.f;
        L.E[idx] = (ok && !exact) ? e[(size_t)col * D + r] : 0.f;
    }
    __syncthreads();
    float* k = ws + (size_t)tile * R * 16;
    fc_eval<KIN>(G, L, t, k, 16, exact, 1.f, -1.f, tid);
    for (int idx = tid; idx < R * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        if (col < B) out[(size_t)col * R + r] = k[idx];
    }
}

}  // namespace rnde
