// rnde_ffjord.h -- TrackedFFJORD with the ConcatSquash dynamics of reference experiments/ffjord_gaussian.jl:48-107: the augmented
// right-hand side [f(z, t); -e . eJ] and the one-launch adaptive Tsit5 solve over it (forward, replay, sampling).
//
// Dynamics: three ConcatSquashLinear layers D -> H -> H -> D with softplus between them, per layer
//     h = (W x + b) .* sig(gw t) + (bw t + bb)
// with the experiment's own sig / softplus (ffjord_gaussian.jl:39-44, accurate expf / log1pf).  The Hutchinson term is the VJP the
// experiment's forw_n_back builds (:98-107): eJ = W1' (s1 .* sig(h1) .* W2' (s2 .* sig(h2) .* W3' (s3 .* e))), trace = e . eJ.
//
// Geometry: ONE workgroup owns the whole batch; thread `tid` owns columns tid, tid + T, ... one after the other.  The controller's
// error norm is a sum over every column, and inside one workgroup that sum is a barrier, not a cross-workgroup meeting: there is no
// spin anywhere in these kernels.  The parameters sit in LDS (every thread reads the same word: broadcast, no bank conflict); the
// three per-column vectors of one evaluation (h1, h2 and a scratch vector of max(H, D) rows) sit in LDS as [row][T] (thread-contiguous,
// conflict free).  The Runge-Kutta state (uprev, unew, stage input, k1..k7) is [row][Bp] in global memory (coalesced, thread-private
// columns: no barrier between the element-wise phases).
// The controller is the chain engine's (advance_state_t, rnde_fwd.h) on a StepParams whose D is the AUGMENTED row count D + 1, so the
// initial-step rule, the PI controller, the step log (StepMeta) and the replay of a given (dt, accept) sequence are those of
// rnde_node_forward / rnde_node_forward_replay.
//
// Kinetic variant (template parameter KIN; TrackedFFJORD{false} called with regularize = true, ffjord.jl:53-66): two more state rows,
//     d lambda1 / dt = sum f^2 (kinetic energy),   d lambda2 / dt = sum eJ^2 (Hutchinson estimate of the Jacobian's Frobenius norm),
// R = D + 3 rows under the same controller.  Both sums fall out of the loops that already form f and eJ: no extra network evaluation.
// Limits: D + 3 <= 64, H <= 64.  The KIN = false instantiations are the code of the plain calls, unchanged.
#pragma once
#include "rnde_fwd.h"

namespace rnde {

constexpr int kFfMaxW = 64;          // the chain engine's width limit: D + 1 <= 64, H <= 64
constexpr int kFfMaxThreads = 512;

struct FfGeo {
    int D, H, P;                     // data rows, hidden width, parameter count
    int off[3];                      // parameter offset of each ConcatSquashLinear (layer_W, layer_B, bias_W, bias_B, gate_W; column-major W)
    int in[3], out[3];
};

__host__ __device__ inline int ff_layer_params(int in, int out) { return out * in + 4 * out; }
__host__ inline FfGeo ff_geo(int D, int H) {
    FfGeo G;
    G.D = D; G.H = H;
    G.in[0] = D; G.out[0] = H; G.in[1] = H; G.out[1] = H; G.in[2] = H; G.out[2] = D;
    int o = 0;
    for (int l = 0; l < 3; ++l) { G.off[l] = o; o += ff_layer_params(G.in[l], G.out[l]); }
    G.P = o;
    return G;
}

// the experiment's sig and softplus (ffjord_gaussian.jl:39-44)
__device__ __forceinline__ float ff_sig(float x) {
    const float t = expf(-fabsf(x));
    return x >= 0.f ? 1.f / (1.f + t) : t / (1.f + t);
}
__device__ __forceinline__ float ff_softplus(float x) { return softplus_f(x); }

// parameter views: W[o][i] = p[off + i * out + o]; then b, bw, bb, gw (each `out` long)
struct FfLayer {
    const float* p; int in, out;
    __device__ __forceinline__ float W(int o, int i) const { return p[i * out + o]; }
    __device__ __forceinline__ float b(int o) const { return p[in * out + o]; }
    __device__ __forceinline__ float bw(int o) const { return p[in * out + out + o]; }
    __device__ __forceinline__ float bb(int o) const { return p[in * out + 2 * out + o]; }
    __device__ __forceinline__ float gw(int o) const { return p[in * out + 3 * out + o]; }
    __device__ __forceinline__ float gate(int o, float t) const { return ff_sig(gw(o) * t); }
    __device__ __forceinline__ float shift(int o, float t) const { return fmaf(bw(o), t, bb(o)); }
};
__device__ __forceinline__ FfLayer ff_layer(const FfGeo& G, const float* p, int l) { return FfLayer{p + G.off[l], G.in[l], G.out[l]}; }

// A per-column vector: element r at v[r * s] (LDS [row][T] or global [row][Bp]).
struct FfVec {
    float* v; int s;
    __device__ __forceinline__ float& operator[](int r) const { return v[(size_t)r * s]; }
};

// One evaluation of the augmented right-hand side for one column.
//   z: the column's D data rows; out: D rows of f, then the trace row -e . eJ (row D);  A, Bv, C: scratch (H, H, max(H, D) rows).
// probe < 0: e is the caller's column (e[i]); probe >= 0: e is the unit vector of row `probe` (the exact trace, sample()).
// Returns e . eJ.  KIN: kin[0] = sum f^2, kin[1] = sum eJ^2 (write_f must be set).
template <bool KIN = false>
__device__ inline float ff_eval(const FfGeo& G, const float* p, float t, FfVec z, FfVec e, int probe, FfVec A, FfVec Bv, FfVec C, FfVec out,
                                bool write_f, float* kin = nullptr) {
    const FfLayer L1 = ff_layer(G, p, 0), L2 = ff_layer(G, p, 1), L3 = ff_layer(G, p, 2);
    const int D = G.D, H = G.H;
    for (int o = 0; o < H; ++o) {
        float acc = L1.b(o);
        for (int i = 0; i < D; ++i) acc = fmaf(L1.W(o, i), z[i], acc);
        A[o] = fmaf(acc, L1.gate(o, t), L1.shift(o, t));                 // h1
    }
    for (int j = 0; j < H; ++j) C[j] = ff_softplus(A[j]);
    for (int o = 0; o < H; ++o) {
        float acc = L2.b(o);
        for (int j = 0; j < H; ++j) acc = fmaf(L2.W(o, j), C[j], acc);
        Bv[o] = fmaf(acc, L2.gate(o, t), L2.shift(o, t));                // h2
    }
    float ke = 0.f, jn = 0.f;
    if (write_f) {
        for (int k = 0; k < H; ++k) C[k] = ff_softplus(Bv[k]);
        for (int i = 0; i < D; ++i) {
            float acc = L3.b(i);
            for (int k = 0; k < H; ++k) acc = fmaf(L3.W(i, k), C[k], acc);
            const float f = fmaf(acc, L3.gate(i, t), L3.shift(i, t));
            out[i] = f;
            if constexpr (KIN) ke = fmaf(f, f, ke);
        }
    }
    // VJP: v3 = s3 .* e ; v2 = s2 .* sig(h2) .* W3' v3 ; v1 = s1 .* sig(h1) .* W2' v2 ; eJ = W1' v1
    for (int i = 0; i < D; ++i) C[i] = L3.gate(i, t) * (probe < 0 ? e[i] : (i == probe ? 1.f : 0.f));
    for (int k = 0; k < H; ++k) {
        float acc = 0.f;
        for (int i = 0; i < D; ++i) acc = fmaf(L3.W(i, k), C[i], acc);
        Bv[k] = acc * ff_sig(Bv[k]) * L2.gate(k, t);
    }
    for (int j = 0; j < H; ++j) {
        float acc = 0.f;
        for (int k = 0; k < H; ++k) acc = fmaf(L2.W(k, j), Bv[k], acc);
        A[j] = acc * ff_sig(A[j]) * L1.gate(j, t);
    }
    float tr = 0.f;
    for (int i = 0; i < D; ++i) {
        float ej = 0.f;
        for (int j = 0; j < H; ++j) ej = fmaf(L1.W(j, i), A[j], ej);
        tr = fmaf(probe < 0 ? e[i] : (i == probe ? 1.f : 0.f), ej, tr);
        if constexpr (KIN) jn = fmaf(ej, ej, jn);
    }
    if constexpr (KIN) { kin[0] = ke; kin[1] = jn; }
    return tr;
}

// The augmented right-hand side of a solve: forward (dir = +1): [f(z, t); -e . eJ];  sampling (dir = -1, tau in [0, t1 - t0]):
// -[f(z, t1 - tau); -tr J] with the exact trace (D VJPs with unit probes, reference jacobian_fn).
struct FfSolveParams {
    StepParams F;                    // the controller's view (F.D = D + 1 rows, F.t0 = 0 / t0, F.t1 = t1 - t0 / t1)
    FfGeo G;
    const float* p;                  // P parameters (global; copied to LDS)
    const float* x;                  // D x B caller layout (column b at x + b D)
    const float* e;                  // D x B caller layout (dir = +1), or NULL (dir = -1: exact trace)
    float* ws;                       // [10][R][Bp]: uprev, unew, stage input, k1..k7
    float* tape;                     // [max_attempts + 1][R][Bp]: uprev of every accepted step, then the end state (NULL: not taped)
    float* logpx;                    // B (dir = +1), may be NULL
    float* x_out;                    // D x B caller layout: the end state's data rows (may be NULL)
    float* norm;                     // [4]: scratch of the initial-step norms (d0, d1 and the third partial for sum_partials: padded to 260)
    int dir, T, Bp;
    float tbase;                     // dir = -1: t1 (the reference's time of tau = 0)
    float* reg;                      // kinetic solves: 2 x B (lambda1 row, then lambda2 row); NULL otherwise
};

// fixed-order workgroup sum, carried in double: wave sums, then the waves in order (the same bits on every thread)
__device__ __forceinline__ double ff_block_sum(float v, float* red, int tid, int T) {
    const int lane = tid & 63, wave = tid >> 6;
    const float w = wave_sum_f(v);
    __syncthreads();
    if (lane == 0) red[wave] = w;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < (T >> 6); ++k) s += (double)red[k];
    return s;
}

// one evaluation for column b: k(:, b) = F(y(:, b), time)  (KIN: forward only, rows D + 1 and D + 2 the two regulariser rates)
template <bool KIN = false>
__device__ inline void ff_rhs(const FfSolveParams& Q, const float* ps, float time, const float* y, float* k, int b, FfVec A, FfVec Bv, FfVec C) {
    const int Bp = Q.Bp, D = Q.G.D;
    const FfVec z{const_cast<float*>(y) + b, Bp}, kk{k + b, Bp};
    if (Q.dir > 0) {
        const FfVec e{const_cast<float*>(Q.e) + (size_t)b * D, 1};
        float kin[2];
        const float tr = ff_eval<KIN>(Q.G, ps, time, z, e, -1, A, Bv, C, kk, true, kin);
        kk[D] = -tr;
        if constexpr (KIN) { kk[D + 1] = kin[0]; kk[D + 2] = kin[1]; }
    } else {
        const float t = Q.tbase - time;
        float tr = 0.f;
        for (int i = 0; i < D; ++i) tr += ff_eval(Q.G, ps, t, z, z, i, A, Bv, C, kk, i == 0);
        for (int i = 0; i < D; ++i) kk[i] = -kk[i];
        kk[D] = tr;
    }
}

// The whole adaptive solve in one launch (one workgroup, Q.T threads).
template <bool KIN>
__global__ __launch_bounds__(kFfMaxThreads) void rnde_ffjord_solve_kernel(const FfSolveParams Q) {
    extern __shared__ float ff_smem[];
    const StepParams& P = Q.F;
    const int tid = threadIdx.x, T = Q.T, lane = tid & 63, Bp = Q.Bp, B = P.B, D = Q.G.D, R = D + (KIN ? 3 : 1);
    const int HS = Q.G.H > D ? Q.G.H : D;
    float* ps = ff_smem;                                   // parameters
    float* red = ff_smem + Q.G.P;                          // 16 wave partials + 8 broadcast doubles
    float* vec = red + 32;                                 // [3][HS][T]
    for (int i = tid; i < Q.G.P; i += T) ps[i] = Q.p[i];
    __syncthreads();
    const FfVec A{vec + tid, T}, Bv{vec + (size_t)HS * T + tid, T}, C{vec + (size_t)2 * HS * T + tid, T};
    const size_t RB = (size_t)R * Bp;
    float* U = Q.ws;  float* UN = Q.ws + RB;  float* Y = Q.ws + 2 * RB;
    auto K = [&](int s) { return Q.ws + (size_t)(3 + s) * RB; };     // s = 0..6: k1..k7
    const float rt = P.reltol, at = P.abstol;
    const double N = (double)R * (double)B;

    // ---- initial state, f(u0), and the initial-step rule (the arithmetic of MW_INIT_A / MW_INIT_B) ----
    float pa = 0.f, pb = 0.f;
    for (int b = tid; b < B; b += T) {
        for (int r = 0; r < D; ++r) U[(size_t)r * Bp + b] = Q.x[(size_t)b * D + r];
        for (int r = D; r < R; ++r) U[(size_t)r * Bp + b] = 0.f;
        ff_rhs<KIN>(Q, ps, P.t0 + 0.f, U, K(0), b, A, Bv, C);
        for (int r = 0; r < R; ++r) {
            const float xv = U[(size_t)r * Bp + b], kv = K(0)[(size_t)r * Bp + b], sk = at + fabsf(xv) * rt;
            const float a = xv / sk, c = kv / sk;
            pa += a * a; pb += c * c;
        }
    }
    const double s0 = ff_block_sum(pa, red, tid, T), s1 = ff_block_sum(pb, red, tid, T);
    float dt0;
    {
        const float d0 = (float)sqrt(s0 / N), d1 = (float)sqrt(s1 / N), dtmax = P.t1 - P.t0;
        int c0 = 0, cl = 0;
        if (d0 < 1e-5f || d1 < 1e-5f) { dt0 = 1e-6f; c0 = 1; }
        else dt0 = (d0 / d1) / 100.f;
        if (dtmax < dt0) { dt0 = dtmax; cl = 1; }
        if (tid == 0) { P.initrec->d0 = d0; P.initrec->d1 = d1; P.initrec->dt0 = dt0; P.initrec->dt0_const = c0; P.initrec->dt0_clamped = cl; }
    }
    float pc = 0.f;
    for (int b = tid; b < B; b += T) {
        for (int r = 0; r < R; ++r) Y[(size_t)r * Bp + b] = U[(size_t)r * Bp + b] + dt0 * K(0)[(size_t)r * Bp + b];
        ff_rhs<KIN>(Q, ps, P.t0 + dt0, Y, K(1), b, A, Bv, C);
        for (int r = 0; r < R; ++r) {
            const float sk = at + fabsf(U[(size_t)r * Bp + b]) * rt;
            const float a = (K(1)[(size_t)r * Bp + b] - K(0)[(size_t)r * Bp + b]) / sk;
            pc += a * a;
        }
    }
    const double s2 = ff_block_sum(pc, red, tid, T);
    if (tid == 0) Q.norm[2] = (float)s2;       // advance_state reads the third initial norm as a one-workgroup partial
    __syncthreads();
    __threadfence_block();
    StepState S = advance_state(P, 0, lane, tid == 0, &P.ctl[0]);
    int n_acc = 0;
    for (int n = 0; !S.done; ++n) {
        const float t = S.t;
        const float dt = (P.t1 - S.t < S.dtp) ? (P.t1 - S.t) : S.dtp;
        float part = 0.f;
        for (int b = tid; b < B; b += T) {
            for (int s = 1; s < 7; ++s) {                  // stage s + 1: input uprev + dt sum_j a_{s+1, j} k_j
                for (int r = 0; r < R; ++r) {
                    const size_t ix = (size_t)r * Bp + b;
                    float acc = 0.f;
                    for (int j = 0; j < s; ++j) acc = fmaf(tsA_rt(s, j), K(j)[ix], acc);
                    const float g = U[ix] + dt * acc;
                    Y[ix] = g;
                    if (s == 6) UN[ix] = g;
                }
                ff_rhs<KIN>(Q, ps, t + kTsC[s] * dt, Y, K(s), b, A, Bv, C);
            }
            for (int r = 0; r < R; ++r) {                  // embedded error estimate, SURVEY.md B.3
                const size_t ix = (size_t)r * Bp + b;
                float E = 0.f;
                for (int j = 0; j < 7; ++j) E += kTsBt[j] * K(j)[ix];
                const float ut = dt * E, sk = at + fmaxf(fabsf(U[ix]), fabsf(UN[ix])) * rt, rr = ut / sk;
                part += rr * rr;
            }
        }
        double xs[3] = {ff_block_sum(part, red, tid, T), 0.0, 0.0};
        const float none[4] = {0.f, 0.f, 0.f, 0.f};
        const StepState Sn = advance_state_t<true>(P, n + 1, lane, tid == 0, &P.ctl[(n + 1) & 1], none, S, xs);
        if (Sn.n_acc > S.n_acc) {                          // accepted: tape uprev, then unew -> uprev, k7 -> k1 (first same as last)
            for (int b = tid; b < B; b += T)
                for (int r = 0; r < R; ++r) {
                    const size_t ix = (size_t)r * Bp + b;
                    if (Q.tape) Q.tape[(size_t)n_acc * RB + ix] = U[ix];
                    U[ix] = UN[ix];
                    K(0)[ix] = K(6)[ix];
                }
            ++n_acc;
        }
        S = Sn;
    }
    if (tid == 0) *P.ctl_final = S;
    // ---- outputs: the end state (taped after the last step), logpx = sum -(log 2 pi + z^2) / 2 - l, the data rows ----
    for (int b = tid; b < B; b += T) {
        float lp = 0.f;
        for (int r = 0; r < R; ++r) {
            const size_t ix = (size_t)r * Bp + b;
            if (Q.tape) Q.tape[(size_t)n_acc * RB + ix] = U[ix];
            if (r < D) {
                const float z = U[ix];
                lp += -(1.8378770664093453f + z * z) * 0.5f;
                if (Q.x_out) Q.x_out[(size_t)b * D + r] = z;
            }
        }
        if (Q.logpx) Q.logpx[b] = lp - U[(size_t)D * Bp + b];
        if constexpr (KIN) { Q.reg[b] = U[(size_t)(D + 1) * Bp + b]; Q.reg[(size_t)B + b] = U[(size_t)(D + 2) * Bp + b]; }
    }
}

// One evaluation of the augmented right-hand side per column (the parity instrument of tests/test_gpu_ffjord.py):
// out: (D + 1) x B caller layout.  probe < 0: Hutchinson with e; else the exact trace (as sample()).  KIN: (D + 3) x B, Hutchinson only.
template <bool KIN>
__global__ __launch_bounds__(256) void rnde_ffjord_feval_kernel(const FfGeo G, const float* __restrict__ p, const float* __restrict__ x,
                                                                const float* __restrict__ e, float t, int B, int exact, float* __restrict__ ws,
                                                                float* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int D = G.D, R = D + (KIN ? 3 : 1), HS = G.H > D ? G.H : D;
    float* w = ws + (size_t)b * (3 * HS + R);                 // per column: A, Bv, C, out
    const FfVec A{w, 1}, Bv{w + HS, 1}, C{w + 2 * HS, 1}, o{w + 3 * HS, 1};
    const FfVec z{const_cast<float*>(x) + (size_t)b * D, 1};
    float tr = 0.f, kin[2];
    if (!exact) tr = ff_eval<KIN>(G, p, t, z, FfVec{const_cast<float*>(e) + (size_t)b * D, 1}, -1, A, Bv, C, o, true, kin);
    else for (int i = 0; i < D; ++i) tr += ff_eval(G, p, t, z, z, i, A, Bv, C, o, i == 0);
    for (int r = 0; r < D; ++r) out[(size_t)b * R + r] = o[r];
    out[(size_t)b * R + D] = -tr;
    if constexpr (KIN) { out[(size_t)b * R + D + 1] = kin[0]; out[(size_t)b * R + D + 2] = kin[1]; }
}

}  // namespace rnde
