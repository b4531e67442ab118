// rnde_bffjord.h -- the reverse sweep of rnde_ffjord_solve_kernel (discretise-then-optimise through every Tsit5 stage of every accepted
// step), in one launch.
//
// What is taped and what is recomputed: the forward tapes uprev of every accepted step (and the end state) plus the step log
// (t, dt, EEst).  The reverse recomputes the seven stages of a step from uprev, then walks them backwards.  Step sizes and times are
// constants of the reverse pass (the chain engine with track_ctrl = track_initdt = 0): the cotangent of a saved value EEst * dt
// reaches the stages through EEst only, with the chain engine's RNDE_REG_ERR reverse of the error norm (rnde_bchainmw.h, part A).
// Rejected attempts contribute nothing.
//
// Once the step sizes are fixed, no column depends on another, so the sweep is one thread per column, as many workgroups as the batch
// needs, and no meeting.  The trace row makes the VJP second order: its reverse differentiates W1' (s1 .* sig(h1) .* ...) and
// sig'(h) = sig(h) (1 - sig(h)) enters.  Parameter cotangents go to a thread-private column of pacc ([P][Bp], plain read-modify-write,
// no atomics); rnde_ffjord_reduce_kernel sums the columns in a fixed order.
//
// Kinetic variant (KIN): F = [f; -e . eJ; sum f^2; sum eJ^2] with the stage cotangent (lz, ll, l1, l2).  The cotangent of f becomes
// lz + 2 l1 f and the cotangent of eJ becomes w = -ll e + 2 l2 eJ; the plain sweep is the case l1 = l2 = 0, where w = c e.  Wherever the
// reverse of tr = e . W1' v1 uses c e the kinetic sweep uses w (v1-bar = W1 w, W1-bar += v1 w'); the rest of the second-order chain is
// the same.  Two more per-column vectors (lz + 2 l1 f, and w) and one more D x H product (eJ) per stage.
#pragma once
#include "rnde_ffjord.h"
#include "rnde_track_rec.h"    // FfStepRec

namespace rnde {

constexpr int kFfVjpVecs = 22;        // per-column vectors of one reverse evaluation (rows: max(H, D))
constexpr int kFfVjpVecsKin = 24;     // the kinetic sweep: + lz + 2 l1 f, + w

struct FfRevParams {
    FfGeo G;
    const float* p;
    const float* e;                   // D x B caller layout
    const float* tape;                // [n_acc + 1][R][Bp]
    const FfStepRec* rec;             // [n_acc]
    const float* logpx_bar;           // B
    float* ws;                        // [21 + 3 + kFfVjpVecs][HR][Bp]
    float* pacc;                      // [P][Bp]
    float* x_bar;                     // D x B caller layout (may be NULL)
    int n_acc, B, Bp;
    float reltol, abstol;
    const float* reg_bar;             // kinetic sweep: 2 x B cotangents of (lambda1, lambda2), or NULL (zeros)
};

__device__ __forceinline__ float ff_dsig(float s) { return s * (1.f - s); }

// per-column vectors in a [slot][row][Bp] workspace: slot k of column b (computed, not held in an array: no private memory)
struct FfSlots {
    float* base; size_t step; int s;
    __device__ __forceinline__ FfVec operator()(int k) const { return FfVec{base + (size_t)k * step, s}; }
};

// ybar[0:D] += (d F / d z)' lam and pacc += (d F / d p)' lam, F = [f(z, t); -e . eJ], lam = (lz; ll)
// KIN: F = [f; -e . eJ; sum f^2; sum eJ^2], lam = (lz; ll; l1; l2)
template <bool KIN = false>
__device__ inline void ff_vjp(const FfGeo& G, const float* p, float t, FfVec z, FfVec e, FfVec lz_in, float ll, FfVec zb, float* pacc, int Bp,
                              const FfSlots V, float l1 = 0.f, float l2 = 0.f) {
    const FfLayer L[3] = {ff_layer(G, p, 0), ff_layer(G, p, 1), ff_layer(G, p, 2)};
    const int D = G.D, H = G.H;
    const FfVec P1 = V(0), H1 = V(1), X1 = V(2), P2 = V(3), H2 = V(4), X2 = V(5), P3 = V(6);
    const FfVec M2 = V(7), V2 = V(8), M1 = V(9), V1 = V(10);
    const FfVec Mb1 = V(11), Hb1 = V(12), SB1 = V(13), Mb2 = V(14), Hb2 = V(15), SB2 = V(16), SB3 = V(17), Pb2 = V(18), Pb1 = V(19);
    const FfVec V3 = V(20), Pb3 = V(21);            // s3 .* e and s3 .* lz (the last layer's gates, evaluated once)
    const FfVec lz = KIN ? V(22) : lz_in, WV = KIN ? V(23) : e;      // KIN: the cotangent of f, and w (the cotangent of eJ)
    const float c = -ll;
    for (int i = 0; i < D; ++i) { const float s3 = L[2].gate(i, t); V3[i] = s3 * e[i]; if constexpr (!KIN) Pb3[i] = s3 * lz[i]; }
    // ---- primal and the trace's forward (the VJP of forw_n_back) ----
    for (int o = 0; o < H; ++o) {
        float acc = L[0].b(o);
        for (int i = 0; i < D; ++i) acc = fmaf(L[0].W(o, i), z[i], acc);
        P1[o] = acc; H1[o] = fmaf(acc, L[0].gate(o, t), L[0].shift(o, t)); X1[o] = ff_softplus(H1[o]);
    }
    for (int o = 0; o < H; ++o) {
        float acc = L[1].b(o);
        for (int j = 0; j < H; ++j) acc = fmaf(L[1].W(o, j), X1[j], acc);
        P2[o] = acc; H2[o] = fmaf(acc, L[1].gate(o, t), L[1].shift(o, t)); X2[o] = ff_softplus(H2[o]);
    }
    for (int i = 0; i < D; ++i) {
        float acc = L[2].b(i);
        for (int k = 0; k < H; ++k) acc = fmaf(L[2].W(i, k), X2[k], acc);
        P3[i] = acc;
        if constexpr (KIN) {           // cotangent of f: lz + 2 l1 f
            const float s3 = L[2].gate(i, t);
            lz[i] = fmaf(2.f * l1, fmaf(acc, s3, L[2].shift(i, t)), lz_in[i]);
            Pb3[i] = s3 * lz[i];
        }
    }
    for (int k = 0; k < H; ++k) {
        float acc = 0.f;
        for (int i = 0; i < D; ++i) acc = fmaf(L[2].W(i, k), V3[i], acc);
        M2[k] = acc; V2[k] = acc * ff_sig(H2[k]) * L[1].gate(k, t);
    }
    for (int j = 0; j < H; ++j) {
        float acc = 0.f;
        for (int k = 0; k < H; ++k) acc = fmaf(L[1].W(k, j), V2[k], acc);
        M1[j] = acc; V1[j] = acc * ff_sig(H1[j]) * L[0].gate(j, t);
    }
    if constexpr (KIN)                 // w = c e + 2 l2 eJ, eJ = W1' v1
        for (int i = 0; i < D; ++i) {
            float ej = 0.f;
            for (int j = 0; j < H; ++j) ej = fmaf(L[0].W(j, i), V1[j], ej);
            WV[i] = fmaf(2.f * l2, ej, c * e[i]);
        }
    // ---- reverse of tr = e . W1' v1 (cotangent c; KIN: of eJ = W1' v1, cotangent w) ----
    for (int j = 0; j < H; ++j) {
        float acc = 0.f;
        for (int i = 0; i < D; ++i) acc = fmaf(L[0].W(j, i), WV[i], acc);
        const float vb = KIN ? acc : c * acc, s = L[0].gate(j, t), sg = ff_sig(H1[j]);
        Mb1[j] = vb * sg * s; Hb1[j] = vb * M1[j] * s * ff_dsig(sg); SB1[j] = vb * M1[j] * sg;
    }
    for (int k = 0; k < H; ++k) {
        float acc = 0.f;
        for (int j = 0; j < H; ++j) acc = fmaf(L[1].W(k, j), Mb1[j], acc);
        const float s = L[1].gate(k, t), sg = ff_sig(H2[k]);
        Mb2[k] = acc * sg * s; Hb2[k] = acc * M2[k] * s * ff_dsig(sg); SB2[k] = acc * M2[k] * sg;
    }
    for (int i = 0; i < D; ++i) {
        float acc = 0.f;
        for (int k = 0; k < H; ++k) acc = fmaf(L[2].W(i, k), Mb2[k], acc);
        SB3[i] = acc * e[i] + lz[i] * P3[i];               // (+ the primal's gate cotangent)
    }
    // ---- reverse of the primal (cotangent lz of f = h3) ----
    for (int k = 0; k < H; ++k) {
        float acc = 0.f;
        for (int i = 0; i < D; ++i) acc = fmaf(L[2].W(i, k), Pb3[i], acc);
        Hb2[k] += acc * ff_sig(H2[k]);
    }
    for (int o = 0; o < H; ++o) { Pb2[o] = Hb2[o] * L[1].gate(o, t); SB2[o] += Hb2[o] * P2[o]; }
    for (int j = 0; j < H; ++j) {
        float acc = 0.f;
        for (int o = 0; o < H; ++o) acc = fmaf(L[1].W(o, j), Pb2[o], acc);
        Hb1[j] += acc * ff_sig(H1[j]);
    }
    for (int o = 0; o < H; ++o) { Pb1[o] = Hb1[o] * L[0].gate(o, t); SB1[o] += Hb1[o] * P1[o]; }
    for (int i = 0; i < D; ++i) {
        float acc = 0.f;
        for (int o = 0; o < H; ++o) acc = fmaf(L[0].W(o, i), Pb1[o], acc);
        zb[i] += acc;
    }
    // ---- parameter cotangents: W_l, b_l, bw_l, bb_l, gw_l ----
    auto acc_p = [&](int q, float v) { pacc[(size_t)q * Bp] += v; };
    for (int l = 0; l < 3; ++l) {
        const int in = G.in[l], out = G.out[l], off = G.off[l];
        for (int o = 0; o < out; ++o) {
            float pb, beta, sb;            // pre-activation cotangent, h cotangent (= shift cotangent), gate cotangent
            if (l == 0) { pb = Pb1[o]; beta = Hb1[o]; sb = SB1[o]; }
            else if (l == 1) { pb = Pb2[o]; beta = Hb2[o]; sb = SB2[o]; }
            else { pb = Pb3[o]; beta = lz[o]; sb = SB3[o]; }
            for (int i = 0; i < in; ++i) {
                float w;
                if (l == 0) w = (KIN ? V1[o] * WV[i] : c * V1[o] * e[i]) + pb * z[i];
                else if (l == 1) w = V2[o] * Mb1[i] + pb * X1[i];
                else w = V3[o] * Mb2[i] + pb * X2[i];
                acc_p(off + i * out + o, w);
            }
            const float s = L[l].gate(o, t);
            acc_p(off + in * out + o, pb);
            acc_p(off + in * out + out + o, beta * t);
            acc_p(off + in * out + 2 * out + o, beta);
            acc_p(off + in * out + 3 * out + o, sb * ff_dsig(s) * t);
        }
    }
}

template <bool KIN>
__global__ __launch_bounds__(256) void rnde_ffjord_reverse_kernel(const FfRevParams Q) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= Q.B) return;
    const FfGeo& G = Q.G;
    const int D = G.D, R = D + (KIN ? 3 : 1), Bp = Q.Bp, HR = (G.H > R ? G.H : R);
    const FfSlots slot{Q.ws + b, (size_t)HR * Bp, Bp};
    const FfSlots Ys{slot.base, slot.step, Bp}, Ks{slot.base + 7 * slot.step, slot.step, Bp}, Kb{slot.base + 14 * slot.step, slot.step, Bp};
    const FfVec UB = slot(21), UBn = slot(22), Yb = slot(23);
    const FfSlots V{slot.base + 24 * slot.step, slot.step, Bp};
    const FfVec e{const_cast<float*>(Q.e) + (size_t)b * D, 1};
    float* pacc = Q.pacc + b;
    for (int q = 0; q < G.P; ++q) pacc[(size_t)q * Bp] = 0.f;
    const size_t RB = (size_t)R * Bp;
    {   // logpx = sum -(log 2 pi + z^2) / 2 - l
        const float g = Q.logpx_bar[b];
        const float* uT = Q.tape + (size_t)Q.n_acc * RB + b;
        for (int r = 0; r < D; ++r) UB[r] = -g * uT[(size_t)r * Bp];
        UB[D] = -g;
        if constexpr (KIN) { UB[D + 1] = Q.reg_bar ? Q.reg_bar[b] : 0.f; UB[D + 2] = Q.reg_bar ? Q.reg_bar[(size_t)Q.B + b] : 0.f; }
    }
    const double N = (double)R * (double)Q.B;
    for (int n = Q.n_acc - 1; n >= 0; --n) {
        const FfStepRec st = Q.rec[n];
        const float t = st.t, dt = st.dt;
        const FfVec U{const_cast<float*>(Q.tape) + (size_t)n * RB + b, Bp};
        // ---- recompute the stages ----
        for (int s = 0; s < 7; ++s) {
            for (int r = 0; r < R; ++r) {
                float acc = 0.f;
                for (int j = 0; j < s; ++j) acc = fmaf(tsA_rt(s, j), Ks(j)[r], acc);
                Ys(s)[r] = U[r] + dt * acc;
            }
            FfVec kk = Ks(s);
            float kin[2];
            kk[D] = -ff_eval<KIN>(G, Q.p, t + kTsC[s] * dt, Ys(s), e, -1, V(0), V(1), V(2), kk, true, kin);
            if constexpr (KIN) { kk[D + 1] = kin[0]; kk[D + 2] = kin[1]; }
        }
        for (int s = 0; s < 7; ++s) for (int r = 0; r < R; ++r) Kb(s)[r] = 0.f;
        for (int r = 0; r < R; ++r) { UBn[r] = 0.f; Yb[r] = UB[r]; }        // Yb: cotangent of unew = stage-7 input
        // ---- A: reverse of the error estimate (the saved value EEst * dt; rnde_bchainmw.h) ----
        if (st.svb != 0.f && st.eest > 0.f) {
            const float coef = (float)(((double)st.svb * (double)dt) / (N * (double)st.eest));
            for (int r = 0; r < R; ++r) {
                float E = 0.f;
                for (int j = 0; j < 7; ++j) E += kTsBt[j] * Ks(j)[r];
                const float up = U[r], un = Ys(6)[r];
                const float au = fabsf(up), an = fabsf(un);
                const bool use_new = !(au > an);
                const float sk = Q.abstol + (use_new ? an : au) * Q.reltol;
                const float rr = dt * E / sk, rb = coef * rr, utb = rb / sk, skb = -rb * rr / sk;
                for (int j = 0; j < 7; ++j) Kb(j)[r] += dt * kTsBt[j] * utb;
                if (use_new) Yb[r] += skb * Q.reltol * (un > 0.f ? 1.f : (un < 0.f ? -1.f : 0.f));
                else UBn[r] += skb * Q.reltol * (up > 0.f ? 1.f : (up < 0.f ? -1.f : 0.f));
            }
        }
        // ---- B: the stages, last to first ----
        for (int s = 6; s >= 0; --s) {
            if (s != 6) for (int r = 0; r < R; ++r) Yb[r] = 0.f;
            if constexpr (KIN) ff_vjp<true>(G, Q.p, t + kTsC[s] * dt, Ys(s), e, Kb(s), Kb(s)[D], Yb, pacc, Bp, V, Kb(s)[D + 1], Kb(s)[D + 2]);
            else ff_vjp(G, Q.p, t + kTsC[s] * dt, Ys(s), e, Kb(s), Kb(s)[D], Yb, pacc, Bp, V);
            for (int r = 0; r < R; ++r) {
                const float y = Yb[r];
                UBn[r] += y;
                for (int j = 0; j < s; ++j) Kb(j)[r] += dt * tsA_rt(s, j) * y;
            }
        }
        for (int r = 0; r < R; ++r) UB[r] = UBn[r];
    }
    if (Q.x_bar) for (int r = 0; r < D; ++r) Q.x_bar[(size_t)b * D + r] = UB[r];
}

// p_bar[q] = sum over columns of pacc[q][.], in column order, carried in double
__global__ __launch_bounds__(256) void rnde_ffjord_reduce_kernel(const float* __restrict__ pacc, int P, int B, int Bp, float* __restrict__ p_bar) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P) return;
    double s = 0.0;
    const float* row = pacc + (size_t)q * Bp;
    for (int b = 0; b < B; ++b) s += (double)row[b];
    p_bar[q] = (float)s;
}

}  // namespace rnde
