// rnde_tile_driver.h -- the tile driver: everything of the engines on the tile layout that does not depend on the dynamics.  One adaptive
// solve, one reverse sweep and one feval kernel, templated on <class Dyn, bool KIN>; the three dynamics are FtDyn (rnde_ffjordt.h /
// rnde_bffjordt.h: TrackedFFJORD over ConcatSquash, engine 1), FcDyn (rnde_ffjordc.h / rnde_bffjordc.h: TrackedFFJORD over Dense chains,
// engine 2) and NtDyn (rnde_node_tile.h: TrackedNeuralODE over a Dense chain, engine 4).  The driver asks the policy's constants, never
// which dynamics it serves.
//
// Layout (rnde_ffjordt.h): one workgroup of four waves per 16 batch columns (a tile); the Runge-Kutta state is [R][Bp] in global memory
// (R = D + Dyn::kAug rows, two more with KIN; each tile touching its own 16 columns), the dynamics keep their parameters and activations in LDS.
//
// Forward solve: the whole adaptive Tsit5 solve in one launch.  Once per attempt every tile forms its partial of the error norm and the tiles
// meet through rnde_meet.h's bounded meet_exchange (one XCD up to 32 tiles, agent scope above): partials are summed in tile order in
// double, so every tile runs the same controller (advance_state_t over R rows) on the same bits, and a solve is bit-identical run to run.
// A meeting that times out raises the abort word and ends the launch; the host reports it by name.  A launch may also carry several
// independent forward solves (rnde_tile_group_solve_kernel: the same body per group, agent scope, a group meeting only with itself).
//
// Reverse sweep: discretise-then-optimise through every Tsit5 stage of every accepted step, step sizes and times constants (track_ctrl =
// track_initdt = 0; the saved value EEst * dt reaches the stages through EEst).  One workgroup per tile, every accepted step in one launch,
// no meeting: once the step log is fixed no column depends on another, and the EEst values come from the step log.  The stage values are
// recomputed from the taped uprev with the forward's own evaluation; the per-column vectors of a stage's VJP live in a per-tile global
// buffer (Dyn::rev_ws_floats; written and read by the same workgroup, L2-resident), no private scratch.  Parameter cotangents accumulate
// in the tile's own row of pacc ([ntiles][P], plain read-modify-write by one lane per entry, no atomics); rnde_tile_reduce_kernel sums
// the tiles in tile order in double.
//
// Tracked reverse sweep (TRK): the PI controller is differentiated as well (track_ctrl = 1; the chain engine's scalar reverse,
// rnde_bchain.h).  The sweep walks ATTEMPTS, last to first; every tile carries the cotangents of (t, the proposed dt, qold) in double
// registers and computes them identically.  A rejected attempt recomputes its stages from the uprev it shares with the accepted attempt
// behind it, has no unew cotangent and ADDS to the running uprev cotangent.  The cotangent of dt needs three sums over the whole batch
// (sum <k_j, k_j-bar>, sum tau_s, sum c_s tau_s with tau_s = <dF/dt at stage s, k_s-bar>): one tile_meet per attempt, in tile order in
// double, under the solve's launch placement (one XCD up to 32 tiles, agent scope above).
//
// What a dynamics policy provides (a plain struct of static members):
//   Geo, Lds                   the geometry (kernel argument: D, P, DP and whatever the dynamics need) and the LDS view (W, X, red, ...; E)
//   kAug                       the rows of the state beyond D: 1 (the log-density row; KIN adds the two regulariser rows) or 0 (never KIN)
//   kProbe                     there is a probe L.E, and with it the exact-trace variants (Q.exact); without one eval and vjp never see L.E
//   kDensity                   the ends of a solve and of a sweep.  true: the solve writes logpx (and reg with KIN) beside x_out, the sweep's
//                              running cotangent is seeded from out_bar = logpx-bar (B) and the last tape record.  false: the solve writes
//                              the end state x_out alone, the sweep is seeded from out_bar = u-bar (R x B), or from zero with SAVE
//   kSpan                      the driver instantiates, for this policy, the saved points (SAVE: the solve writes u(ts) into F.sv_out, the
//                              sweep takes the cotangents of the saved states: out_bar is then R x nsave x B), the reverse of the
//                              initial-step rule behind attempt 0 (Q.track_initdt; scalars: rnde_track_rec.h) and the span cotangents
//                              (t0-bar, t1-bar) with their F_CLAMP and F_DTMAXCLAMP terms.  All of them are written over R rows with
//                              Dyn::eval / Dyn::vjp like the rest, under if constexpr: an instantiation of a policy without kSpan holds none
//   kVjpKdot                   who forms sum <k_s, k_s-bar> of the tracked sweep.  false: the driver, one fmaf chain over the stage values and
//                              cotangents in global memory, carried across the stages, ahead of a stage's first vjp.  true: vjp adds the
//                              stage's partial to *kdot.  The two round differently; a policy keeps the form its tapes were checked with
//   lds(G, smem)               the LDS view over the dynamic shared memory
//   load_params(G, p, W, tid)  parameters into LDS, zero-padded; every thread calls it
//   eval<KIN>(G, L, t, kout, ks, exact, fsign, tsign, scratch, tid)
//                              one evaluation of the right-hand side for the tile's 16 columns.  pre: L.X holds the data rows of the input
//                              ([DP][16], padded rows zero), L.E the probe (Hutchinson; zero where not valid).
//                              out: kout[r * ks + c] = fsign * f_r (r < D); kAug: kout[D * ks + c] = tsign * tr; KIN (Hutchinson only):
//                              kout[(D + 1) * ks + c] = sum f^2, kout[(D + 2) * ks + c] = sum eJ^2.  exact: the exact trace; scratch is
//                              the tile's scratch_floats(G) floats of global memory (NULL where the host has none).  A policy ignores the
//                              arguments it has no use for (NtDyn: exact, the signs, scratch)
//   vjp<KIN>(G, L, t, z, kb, yb, V, pacc, tid, kdot)
//                              yb[0:D] += (dF/dz)' kb and pacc += (dF/dp)' kb; z, kb, yb: [R][16], V: the tile's vector slots.  Returns the
//                              calling thread's share of <dF/dt, kb> over the tile's columns (the tracked sweep sums the shares).  kdot:
//                              NULL outside the tracked sweep; kVjpKdot: *kdot += this thread's share of <F(z, t), kb>.  A non-NULL kdot
//                              is also what asks for the returned share: a policy may form it only then (NtDyn returns 0 otherwise), so a
//                              caller that wants the share and not the sum passes a sum it drops (the initial-step block)
//   lds_floats(G), rev_ws_floats(G, kin), scratch_floats(G)
// Barriers.  The driver writes L.X (and, once, L.E) and calls eval with no barrier of its own: eval places a barrier before its first read
// of L.X or L.E.  Parameters that eval or vjp read ahead of that barrier (FtDyn's gates) load_params makes visible itself, by ending behind
// a barrier; a policy whose eval starts with the barrier (FcDyn, NtDyn) needs none there.  eval and vjp end behind a barrier, every thread
// of the workgroup calls them.
#pragma once
#include "rnde_ffjordt.h"      // the tile layout's constants; rnde_meet.h
#include "rnde_tile_meet.h"    // tile_meet, tile_place
#include "rnde_track_rec.h"    // FfStepRec, FfAttRec, the initial-step rule's scalar reverse
#include "rnde_rev_plan.h"    // SaveRange
#include "rnde_group_plan.h"  // TileGroup

namespace rnde {

template <class Geo>
struct TileSolveParams {
    StepParams F;                    // the controller's view (F.D = R rows; F.ctl / meta / initrec / ctl_final: tile 0's; SAVE: F.sv_t / nsave / sv_out)
    Geo G;
    const float* p;
    const float* x;                  // D x B caller layout
    const float* e;                  // D x B caller layout (Hutchinson), NULL (exact trace, no probe)
    float* ws;                       // [10][R][Bp]: uprev, unew, (unused), k1..k7
    float* tape;                     // [max_attempts + 1][R][Bp] or NULL
    float* logpx;                    // B (dir = +1) or NULL
    float* x_out;                    // D x B caller layout or NULL
    float* norm;                     // [ntiles][8] + 512: each tile's initial-step norms (advance_state reads the third as a one-entry partial)
    InitRec* initrec_t;              // [ntiles]: each tile's copy of the initial-step record (tile 0's is F.initrec)
    StepState* ctl_t;                // [ntiles]: where tiles other than 0 write the state before attempt 0
    float* scratch;                  // [ntiles][Dyn::scratch_floats] (FtDyn: the exact trace's H x H buffer) or NULL
    int exact;                       // the trace row is -tr J (sampling always; a forward solve or replay when the caller asks), not -e . eJ
    Meet meet;                       // three rows per meeting
    unsigned* xcc;                   // [ntiles] (one-XCD meeting: the host checks they agree)
    int xcd_slot;
    int dir, Bp, ntiles;             // dir = -1 (kDensity alone): sampling
    float tbase;                     // dir = -1: t1
    float* reg;                      // kinetic solves: 2 x B (lambda1 row, then lambda2 row); NULL otherwise
};

// (FfAttRec / ff_att_rec, one attempt of the tracked sweep and the scalar reverse of its controller branch: rnde_track_rec.h)

template <class Geo>
struct TileRevParams {
    Geo G;
    const float* p;
    const float* e;                   // D x B caller layout (NULL on an exact tape or without a probe)
    const float* tape;                // [n_acc + 1][R][Bp]
    const FfStepRec* rec;             // [n_acc]
    const float* out_bar;             // the cotangent of the solve's output (kDensity: logpx-bar, B; otherwise u-bar, R x B, SAVE: R x nsave x B)
    float* ws;                        // [ntiles][Dyn::rev_ws_floats]
    float* pacc;                      // [ntiles][P]
    float* x_bar;                     // D x B caller layout (may be NULL)
    int n_acc, B, Bp;
    float reltol, abstol;
    const float* reg_bar;             // kinetic sweep: 2 x B cotangents of (lambda1, lambda2), or NULL (zeros)
    int exact;                        // the tape of an exact-trace forward (never with KIN)
    float* scratch;                   // exact: [ntiles][Dyn::scratch_floats] or NULL, as the solve's
    // the tracked sweep (TRK) alone
    const FfAttRec* att;              // [n_att]
    int n_att;
    Meet meet;                        // three rows per meeting: one per attempt (kSpan: then two for the initial step)
    unsigned* xcc;                    // [ntiles] (one-XCD meeting: the host checks they agree)
    int xcd_slot;
    // TRK with kSpan alone
    int track_initdt;
    InitRec init;                     // the taped solve's initial-step record
    float t0;
    double* tspan_out;                // [2]: (t0-bar, t1-bar), written by tile 0
    // a saving tape (SAVE) alone
    const float* sv_t;                // [nsave]: the tape's own copy of the save times
    const SaveRange* rng;             // the save indices of record n of the sweep's walk: [n_att] by attempt (tracked), [n_acc] by accepted step
    int nsave, save_t0;               // save_t0: index 0 is the start (sv_t[0] == t0), its cotangent goes straight to x_bar
};

// The whole adaptive solve in one launch: forward (dir = +1; Hutchinson, or Q.exact: the exact trace with no probe), replay along P.replay,
// sampling (dir = -1, exact trace, tau = t1 - t).
// SAVE (F.nsave > 0): behind the controller of an accepted attempt every tile writes u(ts) for the save indices [S.next_save, Sn.next_save)
// of the step -- unew itself at the step's end, uprev + dt sum_j b_j(theta) k_j inside it (the Tsit5 dense output, dense_weights; the
// arithmetic of chain_dense_points) -- into F.sv_out (R x nsave x B, caller layout).  Every tile holds the same controller bits, so the
// range is uniform: no meeting and no barrier beyond the loop's.  The save times never enter the controller: a saving solve takes the
// end-state solve's attempts bit for bit.
// The body is tile_solve_body: what tile `tile` of the solve that Q describes does, from the load of the parameters to the last store.  Two
// kernels run it: rnde_tile_solve_kernel (a launch is one solve, Q is the kernel argument) and rnde_tile_group_solve_kernel (a launch is
// several solves, Q is the view of its group that a workgroup builds).
template <class Dyn, bool KIN, bool SAVE>
__device__ __forceinline__ void tile_solve_body(const TileSolveParams<typename Dyn::Geo>& Q, const int tile, float* ft_smem) {
    static_assert((Dyn::kAug || !KIN) && (Dyn::kSpan || !SAVE), "KIN needs the log-density row, SAVE a policy with kSpan");
    const int tid = threadIdx.x, lane = tid & 63;
    const typename Dyn::Geo& G = Q.G;
    constexpr bool AUG = Dyn::kAug > 0;
    const int D = G.D, R = D + Dyn::kAug + (KIN ? 2 : 0), Bp = Q.Bp, B = Q.F.B, col0 = tile * 16;
    StepParams P = Q.F;
    P.initpart = Q.norm + 8 * tile;
    P.initrec = Q.initrec_t + tile;
    const bool lead = tile == 0 && tid == 0;
    const typename Dyn::Lds L = Dyn::lds(G, ft_smem);
    Dyn::load_params(G, Q.p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {     // (the data rows of L.X are rewritten below by the thread that zeroes them)
        if constexpr (Dyn::kProbe) {
            const int r = idx >> 4, col = col0 + (idx & 15);
            L.E[idx] = (!Q.exact && r < D && col < B) ? Q.e[(size_t)col * D + r] : 0.f;
        }
        L.X[idx] = 0.f;
    }
    const size_t RB = (size_t)R * Bp;
    float* U = Q.ws + col0;
    float* UN = Q.ws + RB + col0;
    auto K = [&](int s) { return Q.ws + (size_t)(3 + s) * RB + col0; };
    const int exact = Dyn::kProbe ? Q.exact : 0;
    const bool fwd = !Dyn::kDensity || Q.dir > 0;
    const float fsign = fwd ? 1.f : -1.f, tsign = fwd ? -1.f : 1.f;
    float* scratch = Q.scratch ? Q.scratch + (size_t)tile * Dyn::scratch_floats(G) : nullptr;
    auto eval = [&](float time, float* kout) {
        Dyn::template eval<KIN>(G, L, fwd ? time : Q.tbase - time, kout, Bp, exact, fsign, tsign, scratch, tid);
    };
    const float rt = P.reltol, at = P.abstol;
    const double N = (double)R * (double)B;
    const int nel = R * 16;

    // ---- initial state, f(u0), the initial-step rule (the arithmetic of rnde_ffjord_solve_kernel) ----
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15, col = col0 + c;
        const float v = (r < D && col < B) ? Q.x[(size_t)col * D + r] : 0.f;
        U[(size_t)r * Bp + c] = v;
        if (!AUG || r < D) L.X[r * 16 + c] = v;
    }
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
        if (!AUG || r < D) L.X[r * 16 + c] = U[ix] + dt0 * K(0)[ix];
    }
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
                if (col0 + c < B) P.sv_out[((size_t)(col0 + c) * P.nsave) * R + r] = U[(size_t)r * Bp + c];
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
                if (!AUG || r < D) L.X[r * 16 + c] = g;
                if (s == 6) UN[ix] = g;
            }
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
                    P.sv_out[((size_t)(col0 + c) * P.nsave + si) * R + r] = o;
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
        if ((!AUG || r < D) && col0 + c < B && Q.x_out) Q.x_out[(size_t)(col0 + c) * D + r] = U[ix];
    }
    if constexpr (Dyn::kDensity) {
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
}

template <class Dyn, bool KIN, bool SAVE = false>
__global__ __launch_bounds__(kFtThreads) void rnde_tile_solve_kernel(const TileSolveParams<typename Dyn::Geo> Q) {
    extern __shared__ float ft_smem[];
    int tile;
    if (!tile_place(Q.meet, Q.xcd_slot, Q.xcc, &tile)) return;
    tile_solve_body<Dyn, KIN, SAVE>(Q, tile, ft_smem);
}

// Several independent forward solves ("groups") in one launch (rnde_ffjord_forward_groups; the table: rnde_group_plan.h).  Agent scope, every
// block a tile: block b belongs to the group g with table[g].first_tile <= b < first_tile + ntiles and is tile b - first_tile of it.  It
// builds the group's view of the parameters -- x / e / logpx from the group's first caller column, the workspace from workspace column
// 16 first_tile under the launch's row stride Bp, the group's own controller states, step log, per-tile records, scratch and meeting
// granules (meet_rows sequence numbers of three rows of ntiles granules, behind those of the groups in front), Meet::n = the group's tiles
// -- and runs tile_solve_body on it: the arithmetic of a launch of its own for that batch, bit for bit.  A group meets only with itself and
// leaves when its controller is done; nothing waits for another group.  The abort word is the launch's: a meeting that times out ends
// every group.
template <class Geo>
struct TileGroupParams {
    TileSolveParams<Geo> T;          // the launch: group 0's ranges, the common fields (G, p, exact, the tolerances and the span in F, Bp)
    const TileGroup* table;          // [n_groups], device memory
    int n_groups;
    int meet_rows;                   // sequence numbers of a group's granule range
    int meta_stride;                 // step-log records per group (max_attempts)
    size_t scratch_floats;           // Dyn::scratch_floats per tile (0 without a scratch)
};

template <class Dyn>
__global__ __launch_bounds__(kFtThreads) void rnde_tile_group_solve_kernel(const TileGroupParams<typename Dyn::Geo> Q) {
    static_assert(Dyn::kDensity && Dyn::kAug == 1, "groups are forward solves of the log-density");
    extern __shared__ float ft_smem[];
    const int b = (int)blockIdx.x;
    int g = -1;
    TileGroup me{};
    for (int i = 0; i < Q.n_groups; ++i) {
        const TileGroup t = Q.table[i];
        if (b >= t.first_tile && b < t.first_tile + t.ntiles) { g = i; me = t; }
    }
    if (g < 0) return;               // (a block behind the last group's tiles: the host launches none)
    TileSolveParams<typename Dyn::Geo> V = Q.T;
    const int D = V.G.D;
    V.x += (size_t)me.col0 * D;
    if (V.e) V.e += (size_t)me.col0 * D;
    V.logpx += me.col0;
    V.ws += (size_t)16 * me.first_tile;
    V.F.x = V.x; V.F.B = me.B; V.F.Bn = me.B;
    V.F.ctl += 2 * g; V.F.ctl_final += g; V.F.meta += (size_t)g * Q.meta_stride;
    V.norm += (size_t)8 * me.first_tile;
    V.initrec_t += me.first_tile; V.F.initrec = V.initrec_t;
    V.ctl_t += me.first_tile;
    if (V.scratch) V.scratch += (size_t)me.first_tile * Q.scratch_floats;
    V.meet.xch += (size_t)Q.meet_rows * 3 * me.first_tile;
    V.meet.n = me.ntiles; V.meet.global = 1;
    V.ntiles = me.ntiles;
    tile_solve_body<Dyn, false, false>(V, b - me.first_tile, ft_smem);
}

// sum[0] += the sum of logpx[0 .. n) in double, count[0] += n: what a likelihood pass accumulates over its calls.  One workgroup of 256
// threads, one fixed order: thread t adds logpx[t], logpx[t + 256], logpx[t + 512], ... in that order into a double that starts at zero;
// the 256 partials are then folded in LDS, entry i += entry i + s for s = 128, 64, ..., 1; thread 0 adds the total to *sum and n to
// *count with a plain load and store.  No atomics, so two runs over the same values give the same bits.
static __global__ __launch_bounds__(256) void rnde_group_sum_kernel(const float* __restrict__ logpx, int n, double* sum, long long* count) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) s += (double)logpx[i];
    part[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) { *sum += part[0]; *count += (long long)n; }
}

// The reverse sweep of the taped solve; KIN: the stage cotangent is (lz, ll, l1, l2) over R = D + 3 rows.
// Q.exact (the tape of an exact-trace forward): the stages are recomputed with the exact trace, and the trace row's cotangent goes through
// -tr J = -sum_i e_i . (e_i J) over the unit probes.  Dyn::vjp is linear in kb, so a stage takes D + 1 calls of it: one with L.E = 0 and the
// whole kb (the trace row is quadratic in the probe and gives nothing there), then one per unit probe with kb cut down to its trace row.
// TRK: the tracked sweep (the header); launched as the solve is (MeetRes::grid), one loop iteration per attempt; with kSpan the initial
// step follows: f0, u1 = x + dt0 f0 and f1 are recomputed, two VJPs and two more meetings reverse the rule, and the cotangent of t in front
// of attempt 0 and the clamps (dt = t1 - t, dtp' = t1 - t0) give (t0-bar, t1-bar).
// SAVE: a saving tape.  The only outputs are the saved points: the running uprev cotangent starts at zero, and behind the seeds of an
// accepted attempt the cotangent of each of its save indices (Q.rng, formed on the host by save_plan) enters -- at the step's end into the
// unew cotangent, inside the step into the uprev cotangent and, times dt b_j(theta), into every stage cotangent (the reverse of the dense
// output, rnde_bchain.h).  TRK adds the theta terms to the attempt's sums: -<u_s-bar, sum_j b_j'(theta) k_j> to the t sum and theta times it
// to the dt sum (theta = (ts - t) / dt); the dt b_j part of the dt cotangent is in sum <k_j, k_j-bar> already.  The meeting carries them:
// no meeting is added.  The cotangent of index 0 under save_start goes straight to x-bar.
template <class Dyn, bool KIN, bool TRK = false, bool SAVE = false>
__global__ __launch_bounds__(kFtThreads) void rnde_tile_reverse_kernel(const TileRevParams<typename Dyn::Geo> Q) {
    static_assert((Dyn::kAug || !KIN) && (Dyn::kSpan || !SAVE), "KIN needs the log-density row, SAVE a policy with kSpan");
    extern __shared__ float ft_smem[];
    const typename Dyn::Geo& G = Q.G;
    int tile = (int)blockIdx.x;
    if constexpr (TRK)
        if (!tile_place(Q.meet, Q.xcd_slot, Q.xcc, &tile)) return;
    constexpr bool AUG = Dyn::kAug > 0, SPAN = TRK && Dyn::kSpan;
    const int tid = threadIdx.x, D = G.D, R = D + Dyn::kAug + (KIN ? 2 : 0), Bp = Q.Bp, col0 = tile * 16, nel = R * 16;
    const typename Dyn::Lds L = Dyn::lds(G, ft_smem);
    const int exact = (KIN || !Dyn::kProbe) ? 0 : Q.exact;
    Dyn::load_params(G, Q.p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        if constexpr (Dyn::kProbe) {
            const int r = idx >> 4, col = col0 + (idx & 15);
            L.E[idx] = (!exact && r < D && col < Q.B) ? Q.e[(size_t)col * D + r] : 0.f;
        }
        L.X[idx] = 0.f;
    }
    float* scratch = (exact && Q.scratch) ? Q.scratch + (size_t)tile * Dyn::scratch_floats(G) : nullptr;
    float* ws = Q.ws + (size_t)tile * Dyn::rev_ws_floats(G, KIN);
    const size_t RS = (size_t)nel;
    auto Ys = [&](int s) { return ws + (size_t)s * RS; };
    auto Ks = [&](int s) { return ws + (size_t)(7 + s) * RS; };
    auto Kb = [&](int s) { return ws + (size_t)(14 + s) * RS; };
    float *UB = ws + 21 * RS, *UBn = ws + 22 * RS, *Yb = ws + 23 * RS, *V = ws + 24 * RS;
    float* pacc = Q.pacc + (size_t)tile * G.P;
    for (int q = tid; q < G.P; q += kFtThreads) pacc[q] = 0.f;
    const size_t RB = (size_t)R * Bp;
    for (int idx = tid; idx < nel; idx += kFtThreads) {     // the seeds (kDensity: logpx = sum -(log 2 pi + z^2) / 2 - l)
        const int r = idx >> 4, c = idx & 15, col = col0 + c;
        float v = 0.f;
        if (col < Q.B) {
            if constexpr (Dyn::kDensity) {
                const float g = Q.out_bar[col];
                v = r < D ? -g * Q.tape[(size_t)Q.n_acc * RB + (size_t)r * Bp + col] : -g;
                if constexpr (KIN)
                    if (r > D) v = Q.reg_bar ? Q.reg_bar[(size_t)(r - D - 1) * Q.B + col] : 0.f;
            } else if constexpr (!SAVE) {
                v = Q.out_bar[(size_t)col * R + r];
            }
        }
        UB[idx] = v;
    }
    // (Nothing below needs this barrier for its data: UB[idx] and L.X[idx] are next touched by the thread that wrote them, pacc and L.E behind
    // the first eval's barriers.  It is here for the compiler: with the stores above fenced off, the uniform loads of the loop -- Q.rec[n],
    // Q.att[n], Q.rng[n] -- are scalar loads; without it they are vector loads whose vmcnt waits run through the whole stage loop.)
    __syncthreads();
    const double N = (double)R * (double)Q.B;
    double tb = 0.0, dtpb = 0.0, qoldb = 0.0;      // TRK: the cotangents of (t, the proposed dt, qold) behind attempt n
    [[maybe_unused]] double t1b = 0.0, t0b = 0.0;  // SPAN: the cotangents of the span
    for (int n = (TRK ? Q.n_att : Q.n_acc) - 1; n >= 0; --n) {
        FfStepRec st;
        FfAttRec a;                   // TRK: the attempt's record, loaded once
        int flags = F_ACCEPT, urec = n;
        if constexpr (TRK) { a = Q.att[n]; st.t = a.t; st.dt = a.dt; st.eest = a.eest; st.svb = 0.f; flags = a.flags; urec = a.rec; }
        else st = Q.rec[n];
        const float t = st.t, dt = st.dt;
        const bool accepted = (flags & F_ACCEPT) != 0;
        const float* U = Q.tape + (size_t)urec * RB + col0;
        // ---- recompute the stages ----
        for (int s = 0; s < 7; ++s) {
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                float acc = 0.f;
                for (int j = 0; j < s; ++j) acc = fmaf(tsA_rt(s, j), Ks(j)[idx], acc);
                const float y = U[(size_t)r * Bp + c] + dt * acc;
                Ys(s)[idx] = y;
                if (!AUG || r < D) L.X[idx] = y;
            }
            Dyn::template eval<KIN>(G, L, t + kTsC[s] * dt, Ks(s), 16, exact, 1.f, -1.f, scratch, tid);
        }
        for (int idx = tid; idx < nel; idx += kFtThreads) {
            for (int s = 0; s < 7; ++s) Kb(s)[idx] = 0.f;
            UBn[idx] = 0.f;
            Yb[idx] = accepted ? UB[idx] : 0.f;               // cotangent of unew = stage-7 input (a rejected attempt has none)
        }
        float pS = 0.f, ptau = 0.f, pctau = 0.f;              // TRK: this thread's shares of the three sums of the dt cotangent
        if constexpr (SAVE) {         // ---- the saved points of this step (every array below is touched by its entry's owner thread alone: no barrier) ----
            const SaveRange rg = Q.rng[n];
            for (int si = rg.lo; si < rg.hi; ++si) {
                const float ts = Q.sv_t[si], th = (ts - t) / dt;
                const bool at_end = ts == t + dt;
                float bw[7], dbw[7];
                dense_weights(th, bw);
                if constexpr (TRK) dense_weights_deriv(th, dbw);
                for (int idx = tid; idx < nel; idx += kFtThreads) {
                    const int r = idx >> 4, col = col0 + (idx & 15);
                    if (col >= Q.B) continue;
                    const float ub = Q.out_bar[((size_t)col * Q.nsave + si) * R + r];
                    if (at_end) { Yb[idx] += ub; continue; }
                    UBn[idx] += ub;
#pragma unroll
                    for (int j = 0; j < 7; ++j) Kb(j)[idx] += dt * bw[j] * ub;      // (unrolled: bw, dbw stay in registers)
                    if constexpr (TRK) {
                        float dacc = dbw[0] * Ks(0)[idx];
#pragma unroll
                        for (int j = 1; j < 7; ++j) dacc += dbw[j] * Ks(j)[idx];
                        const float v = -ub * dacc;
                        ptau += v; pctau = fmaf(th, v, pctau);
                    }
                }
            }
        }
        // ---- TRK: the scalar reverse of the controller (FfAttRec); SPAN: dtp' = t1 - t0 under F_DTMAXCLAMP ----
        double eb = 0.0, dtb_pre = 0.0, qoldb_in = 0.0;
        if constexpr (TRK) {
            eb = a.e0 + a.e_dtp * dtpb + a.e_q * qoldb;
            dtb_pre = a.d0 + a.d_t * tb + a.d_dtp * dtpb;
            qoldb_in = a.c_dtp * dtpb + a.c_q * qoldb;
            if constexpr (SPAN)
                if (accepted && (flags & F_DTMAXCLAMP)) { t1b += dtpb; t0b -= dtpb; }
        }
        // ---- A: reverse of the error estimate (the saved value EEst * dt; rnde_bffjord.h.  TRK: every attempt, with the coefficient eb) ----
        if (TRK ? (eb != 0.0 && st.eest > 0.f) : (st.svb != 0.f && st.eest > 0.f)) {
            const float coef = TRK ? (float)(eb / (N * (double)st.eest)) : (float)(((double)st.svb * (double)dt) / (N * (double)st.eest));
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                if (col0 + (idx & 15) >= Q.B) continue;
                float E = 0.f;
                for (int j = 0; j < 7; ++j) E += kTsBt[j] * Ks(j)[idx];
                const float up = U[(size_t)(idx >> 4) * Bp + (idx & 15)], un = Ys(6)[idx];
                const float au = fabsf(up), an = fabsf(un);
                const bool use_new = !(au > an);
                const float sk = Q.abstol + (use_new ? an : au) * Q.reltol;
                const float rr = dt * E / sk, rb = coef * rr, utb = rb / sk, skb = -rb * rr / sk;
                for (int j = 0; j < 7; ++j) Kb(j)[idx] += dt * kTsBt[j] * utb;
                if (use_new) Yb[idx] += skb * Q.reltol * (un > 0.f ? 1.f : (un < 0.f ? -1.f : 0.f));
                else UBn[idx] += skb * Q.reltol * (up > 0.f ? 1.f : (up < 0.f ? -1.f : 0.f));
            }
        }
        __syncthreads();
        // ---- B: the stages, last to first ----
        for (int s = 6; s >= 0; --s) {
            if (s != 6) {
                for (int idx = tid; idx < nel; idx += kFtThreads) Yb[idx] = 0.f;
                __syncthreads();
            }
            const int npass = exact ? D + 1 : 1;
            if constexpr (TRK && !Dyn::kVjpKdot)      // <k_s, k_s-bar>: k_s-bar is complete here (an exact sweep's pass 1 cuts it down)
                for (int idx = tid; idx < nel; idx += kFtThreads) pS = fmaf(Ks(s)[idx], Kb(s)[idx], pS);
            for (int pass = 0; pass < npass; ++pass) {
                if (exact) {          // pass 0: L.E = 0, the whole kb; pass i: the unit probe e_i, kb's trace row alone (Kb(s) is not read again)
                    if constexpr (Dyn::kProbe) {
                        __syncthreads();
                        for (int idx = tid; idx < G.DP * 16; idx += kFtThreads)
                            L.E[idx] = ((idx >> 4) == pass - 1 && col0 + (idx & 15) < Q.B) ? 1.f : 0.f;
                        if (pass == 1)
                            for (int idx = tid; idx < D * 16; idx += kFtThreads) Kb(s)[idx] = 0.f;
                        __syncthreads();
                    }
                }
                const float ts = Dyn::template vjp<KIN>(G, L, t + kTsC[s] * dt, Ys(s), Kb(s), Yb, V, pacc, tid, TRK ? &pS : nullptr);
                if constexpr (TRK) { ptau += ts; pctau = fmaf(kTsC[s], ts, pctau); }
            }
            // (exact: L.E is left holding the last unit probe; harmless, no dynamics' eval reads L.E when exact is set)
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float y = Yb[idx];
                UBn[idx] += y;
                for (int j = 0; j < s; ++j) Kb(j)[idx] += dt * tsA_rt(s, j) * y;
            }
            __syncthreads();
        }
        for (int idx = tid; idx < nel; idx += kFtThreads) UB[idx] = accepted ? UBn[idx] : UB[idx] + UBn[idx];
        __syncthreads();
        if constexpr (TRK) {          // the meeting, then the scalar tail (finish_attempt_scalars_sums, rnde_bwd.h): dt = min(dtp, t1 - t), t' = t + dt
            double xs[3];
            if (!tile_meet(Q.meet, L.red, n, pS, ptau, pctau, xs, tile, tid)) return;
            const double dtb = dtb_pre + xs[0] / (double)dt + xs[2];
            tb += xs[1];
            if (flags & F_CLAMP) {
                if constexpr (SPAN) t1b += dtb;
                tb -= dtb; dtpb = 0.0;
            } else dtpb = dtb;
            qoldb = qoldb_in;
        }
    }
    if constexpr (SPAN) {
        if (Q.track_initdt) {         // ---- the initial-step rule behind attempt 0 (rnde_bchain_init_kernel's two phases; scalars: rnde_track_rec.h) ----
            const InitRec& ir = Q.init;
            const float dt0 = ir.dt0, rt = Q.reltol, at = Q.abstol;
            const float* X0 = Q.tape + col0;                  // tape record 0: x (padded columns zero)
            const InitBar1 b1 = init_rev_phase1(ir, dtpb, N);
            float drop = 0.f;                                 // (<F, kb> of the two VJPs below enters nothing)
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float xv = X0[(size_t)(idx >> 4) * Bp + (idx & 15)];
                Ys(0)[idx] = xv;
                if (!AUG || (idx >> 4) < D) L.X[idx] = xv;
            }
            Dyn::template eval<KIN>(G, L, Q.t0 + 0.f, Ks(0), 16, exact, 1.f, -1.f, scratch, tid);      // f0 = f(x, t0)
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float y = Ys(0)[idx] + dt0 * Ks(0)[idx];
                Ys(1)[idx] = y;
                if (!AUG || (idx >> 4) < D) L.X[idx] = y;
            }
            Dyn::template eval<KIN>(G, L, Q.t0 + dt0, Ks(1), 16, exact, 1.f, -1.f, scratch, tid);      // f1 = f(u1, t0 + dt0)
            const float cw = (float)b1.coef_w;
            for (int idx = tid; idx < nel; idx += kFtThreads) {              // phase 1: f1-bar = coef_w (f1 - f0) / sk^2
                float f1b = 0.f;
                if (col0 + (idx & 15) < Q.B) { const float sk = at + fabsf(Ys(0)[idx]) * rt; f1b = cw * ((Ks(1)[idx] - Ks(0)[idx]) / sk) / sk; }
                Kb(1)[idx] = f1b;
                Yb[idx] = 0.f;
            }
            __syncthreads();
            float ptau = Dyn::template vjp<KIN>(G, L, Q.t0 + dt0, Ys(1), Kb(1), Yb, V, pacc, tid, &drop);
            float pdot = 0.f;
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float g = Yb[idx];                                     // u1-bar
                UBn[idx] = g;
                pdot = fmaf(g, Ks(0)[idx], pdot);
            }
            double xs[3];
            if (!tile_meet(Q.meet, L.red, Q.n_att, pdot, ptau, 0.f, xs, tile, tid)) return;
            const InitBar2 b2 = init_rev_phase2(ir, b1, xs[0], xs[1]);
            t0b += b2.t0b; t1b += b2.t1b;
            const float cv = ir.d1 > 0.f ? (float)(b2.d1b / (N * (double)ir.d1)) : 0.f;
            const float cz = ir.d0 > 0.f ? (float)(b2.d0b / (N * (double)ir.d0)) : 0.f;
            for (int idx = tid; idx < nel; idx += kFtThreads) {              // phase 2: f0-bar = dt0 u1-bar + (v-bar - w-bar) / sk, the x-bar terms of the three norms
                const float xv = Ys(0)[idx], f0 = Ks(0)[idx], ub1 = UBn[idx];
                float f0b = dt0 * ub1, u0b = UB[idx] + ub1;
                if (col0 + (idx & 15) < Q.B) {
                    const float sk = at + fabsf(xv) * rt;
                    const float w = (Ks(1)[idx] - f0) / sk, v = f0 / sk, z = xv / sk;
                    const float wb = cw * w, vb = cv * v, zb = cz * z;
                    const float skb = -(wb * w + vb * v + zb * z) / sk;
                    f0b += (vb - wb) / sk;
                    u0b += zb / sk + skb * rt * (xv > 0.f ? 1.f : (xv < 0.f ? -1.f : 0.f));
                }
                Kb(0)[idx] = f0b;
                UB[idx] = u0b;
                Yb[idx] = 0.f;
            }
            __syncthreads();
            ptau = Dyn::template vjp<KIN>(G, L, Q.t0 + 0.f, Ys(0), Kb(0), Yb, V, pacc, tid, &drop);
            for (int idx = tid; idx < nel; idx += kFtThreads) UB[idx] += Yb[idx];
            if (!tile_meet(Q.meet, L.red, Q.n_att + 1, ptau, 0.f, 0.f, xs, tile, tid)) return;
            t0b += xs[0];
        }
        if (tile == 0 && tid == 0) { Q.tspan_out[0] = t0b + tb; Q.tspan_out[1] = t1b; }      // t-bar in front of attempt 0 is t0's
    }
    if (Q.x_bar)
        for (int idx = tid; idx < nel; idx += kFtThreads) {
            const int r = idx >> 4, col = col0 + (idx & 15);
            if ((AUG && r >= D) || col >= Q.B) continue;
            if constexpr (SAVE) {
                float v = UB[idx];
                if (Q.save_t0) v += Q.out_bar[((size_t)col * Q.nsave) * R + r];
                Q.x_bar[(size_t)col * D + r] = v;
            } else Q.x_bar[(size_t)col * D + r] = UB[idx];
        }
}

// One evaluation of the right-hand side per column (the parity instrument): out R x B caller layout, the trace row -e . eJ (exact: -tr J).
// One workgroup per tile; ws: [ntiles][R][16].  KIN: (D + 3) x B, Hutchinson only.
template <class Dyn, bool KIN>
__global__ __launch_bounds__(kFtThreads) void rnde_tile_feval_kernel(const typename Dyn::Geo G, const float* __restrict__ p, const float* __restrict__ x,
                                                                    const float* __restrict__ e, float t, int B, int exact, float* __restrict__ ws,
                                                                    float* __restrict__ scratch, float* __restrict__ out) {
    extern __shared__ float ft_smem[];
    const int tile = blockIdx.x, tid = threadIdx.x, D = G.D, R = D + Dyn::kAug + (KIN ? 2 : 0), col0 = tile * 16;
    const typename Dyn::Lds L = Dyn::lds(G, ft_smem);
    Dyn::load_params(G, p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        const bool ok = r < D && col < B;
        L.X[idx] = ok ? x[(size_t)col * D + r] : 0.f;
        if constexpr (Dyn::kProbe) L.E[idx] = (ok && !exact) ? e[(size_t)col * D + r] : 0.f;
    }
    float* k = ws + (size_t)tile * R * 16;
    Dyn::template eval<KIN>(G, L, t, k, 16, exact, 1.f, -1.f, scratch ? scratch + (size_t)tile * Dyn::scratch_floats(G) : nullptr, tid);
    for (int idx = tid; idx < R * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        if (col < B) out[(size_t)col * R + r] = k[idx];
    }
}

// p_bar[q] = sum over tiles of pacc[tile][q], in tile order, carried in double (static: both translation units of the tile layout hold it)
static __global__ __launch_bounds__(256) void rnde_tile_reduce_kernel(const float* __restrict__ pacc, int P, int ntiles, float* __restrict__ p_bar) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P) return;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s += (double)pacc[(size_t)t * P + q];
    p_bar[q] = (float)s;
}

}  // namespace rnde
