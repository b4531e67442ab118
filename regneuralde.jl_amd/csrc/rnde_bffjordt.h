// rnde_bffjordt.h -- the reverse sweep of rnde_ffjordt_solve_kernel: what rnde_bffjord.h differentiates (discretise-then-optimise through every
// Tsit5 stage of every accepted step, step sizes and times constants: track_ctrl = track_initdt = 0; the saved value EEst * dt reaches the
// stages through EEst), with the tiled engine's geometry.
//
// One workgroup per 16-column tile, every accepted step in one launch, no meeting: once the step log is fixed no column depends on another,
// and the EEst values come from the step log.  The stage values are recomputed from the taped uprev with the forward's own evaluation
// (rnde_ffjordt.h ft_eval, activations in LDS).  The second-order VJP of a stage needs some 27 per-column vectors; next to the resident
// weights they do not fit in LDS at the tabular widths, so they live in a per-tile global buffer (written and read by the same workgroup,
// L2-resident); no private scratch.  Every product, the weight cotangents included (outer products over the tile's 16 columns, k = 2 x 16),
// runs on the matrix cores.  Parameter cotangents accumulate in the tile's own row of pacc ([ntiles][P], plain read-modify-write by one lane
// per entry, no atomics); rnde_ffjordt_reduce_kernel sums the tiles in tile order in double.
//
// Kinetic variant (KIN; the arithmetic of rnde_bffjord.h): the stage cotangent is (lz, ll, l1, l2) over R = D + 3 rows.  The cotangent of f,
// lz + 2 l1 f, is formed in the epilogue of the layer-3 product; w = -ll e + 2 l2 eJ needs eJ = W1' v1, one more transposed product once v1
// is known, and W1 w replaces c (W1 e).  Both are two more vector slots of the per-tile global buffer: no LDS beyond the plain kernel's.
#pragma once
#include "rnde_bffjord.h"      // FfStepRec, ff_dsig
#include "rnde_ffjordt.h"

namespace rnde {

constexpr int kFtVjpVecs = 27;
constexpr int kFtVjpVecsKin = 28;      // + w (the cotangent of eJ)

struct FtRevParams {
    FtGeo G;
    const float* p;
    const float* e;                   // D x B caller layout
    const float* tape;                // [n_acc + 1][R][Bp]
    const FfStepRec* rec;             // [n_acc]
    const float* logpx_bar;           // B
    float* ws;                        // [ntiles][ft_rev_ws_floats]
    float* pacc;                      // [ntiles][P]
    float* x_bar;                     // D x B caller layout (may be NULL)
    int n_acc, B, Bp;
    float reltol, abstol;
    const float* reg_bar;             // kinetic sweep: 2 x B cotangents of (lambda1, lambda2), or NULL (zeros)
};

__host__ __device__ inline size_t ft_rev_ws_floats(const FtGeo& G, bool kin = false) {
    const int R = G.D + (kin ? 3 : 1), FP = G.HP > G.DP ? G.HP : G.DP;
    return (size_t)24 * R * 16 + (size_t)(kin ? kFtVjpVecsKin : kFtVjpVecs) * FP * 16;
}

// dW[o][i] += sum_c A1[o][c] B1[i][c] + A2[o][c] B2[i][c] (all [feature][16]) into pw[i * out + o]; output tiles dealt to the waves
__device__ __forceinline__ void ft_wgrad(const float* A1, const float* B1, const float* A2, const float* B2, int outp, int inp, int out, int in,
                                         float* pw, int wave, int lane) {
    const int c = lane & 15, g = lane >> 4, nti = inp >> 4, nt = (outp >> 4) * nti;
    for (int tt = wave; tt < nt; tt += kFtWaves) {
        const int mo = tt / nti, mi = tt - mo * nti;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int ao = (16 * mo + c) * 16 + g, bo = (16 * mi + c) * 16 + g;
#pragma unroll
        for (int kc = 0; kc < 16; kc += 4) {
            acc = mfma16(A1[ao + kc], B1[bo + kc], acc);
            acc = mfma16(A2[ao + kc], B2[bo + kc], acc);
        }
        const int i = 16 * mi + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = 16 * mo + 4 * g + j;
            if (o < out && i < in) pw[(size_t)i * out + o] += acc[j];
        }
    }
}

// yb[0:D] += (dF/dz)' lam and pacc += (dF/dp)' lam for the tile's 16 columns, F = [f(z, t); -e . eJ], lam = (lz; ll) = kb.
// z: the stage input ([R][16]), kb: its cotangent ([R][16]), yb: [R][16], V: the tile's vector slots.  Ends behind a barrier.
// KIN: F = [f; -e . eJ; sum f^2; sum eJ^2], lam = (lz; ll; l1; l2).
template <bool KIN = false>
__device__ __forceinline__ void ft_vjp(const FtGeo& G, const FtLds& L, float t, const float* z, const float* kb, float* yb, float* V, float* pacc, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, H = G.H, HP = G.HP, DP = G.DP;
    const int FP = HP > DP ? HP : DP;
    auto vec = [&](int k) { return V + (size_t)k * FP * 16; };
    float *ZP = vec(0), *LZ = vec(1), *P1 = vec(2), *SG1 = vec(3), *X1 = vec(4), *VB1 = vec(5), *P2 = vec(6), *SG2 = vec(7), *X2 = vec(8);
    float *P3 = vec(9), *V3 = vec(10), *Pb3 = vec(11), *T2 = vec(12), *M2 = vec(13), *V2 = vec(14), *M1 = vec(15), *V1 = vec(16);
    float *CV1 = vec(17), *Mb1 = vec(18), *Hb1 = vec(19), *SB1 = vec(20), *Mb2 = vec(21), *Hb2 = vec(22), *Pb2 = vec(23), *SB2 = vec(24);
    float *SB3 = vec(25), *Pb1 = vec(26);
    float* WV = KIN ? vec(27) : nullptr;                 // w = c e + 2 l2 eJ
    float *l1v = L.red + 96, *l2v = L.red + 112;        // per column: the cotangents of the two regulariser rows
    const float *W1 = L.W + G.woff[0], *W2 = L.W + G.woff[1], *W3 = L.W + G.woff[2];
    const float *g1 = L.GT, *g2 = L.GT + HP, *g3 = L.GT + 2 * HP;
    float* cv = L.red + 80;           // per column: c = -(cotangent of the trace row)
    ft_gates(G, L.W, L.GT, t, tid);
    for (int idx = tid; idx < DP * 16; idx += kFtThreads) {
        const int r = idx >> 4;
        ZP[idx] = r < D ? z[idx] : 0.f;
        LZ[idx] = r < D ? kb[idx] : 0.f;
    }
    if (tid < 16) cv[tid] = -kb[D * 16 + tid];
    if constexpr (KIN)
        if (tid < 16) { l1v[tid] = kb[(D + 1) * 16 + tid]; l2v[tid] = kb[(D + 2) * 16 + tid]; }
    __syncthreads();
    // primal layer 1, and W1 e for the reverse of the trace
    ft_fwd(W1, G.ld[0], G.inp[0], G.outp[0], ZP, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 0, 0), *bw = ft_vec(G, L.W, 0, 1), *bb = ft_vec(G, L.W, 0, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j, ix = o * 16 + c;
            float p1 = 0.f, sg = 0.f, x1 = 0.f;
            if (o < H) { p1 = v[j] + b[o]; const float h = fmaf(p1, g1[o], fmaf(bw[o], t, bb[o])); sg = ff_sig(h); x1 = ff_softplus(h); }
            P1[ix] = p1; SG1[ix] = sg; X1[ix] = x1;
        }
    });
    if constexpr (!KIN)
        ft_fwd(W1, G.ld[0], G.inp[0], G.outp[0], L.E, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) VB1[(r0 + j) * 16 + c] = cv[c] * v[j];
        });
    for (int idx = tid; idx < DP * 16; idx += kFtThreads) {
        const float s3 = g3[idx >> 4];
        V3[idx] = s3 * L.E[idx];
        if constexpr (!KIN) Pb3[idx] = s3 * LZ[idx];
    }
    __syncthreads();
    ft_fwd(W2, G.ld[1], G.inp[1], G.outp[1], X1, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 1, 0), *bw = ft_vec(G, L.W, 1, 1), *bb = ft_vec(G, L.W, 1, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j, ix = o * 16 + c;
            float p2 = 0.f, sg = 0.f, x2 = 0.f;
            if (o < H) { p2 = v[j] + b[o]; const float h = fmaf(p2, g2[o], fmaf(bw[o], t, bb[o])); sg = ff_sig(h); x2 = ff_softplus(h); }
            P2[ix] = p2; SG2[ix] = sg; X2[ix] = x2;
        }
    });
    __syncthreads();
    // primal layer 3 (pre-gate), the trace's m2 = W3' (g3 .* e), and W3' (g3 .* lz) for the primal reverse
    ft_fwd(W3, G.ld[2], G.inp[2], G.outp[2], X2, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 2, 0), *bw = ft_vec(G, L.W, 2, 1), *bb = ft_vec(G, L.W, 2, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j, ix = o * 16 + c;
            const float p3 = o < D ? v[j] + b[o] : 0.f;
            P3[ix] = p3;
            if constexpr (KIN) {       // the cotangent of f: lz + 2 l1 f (this lane owns the entry)
                const float lz = o < D ? fmaf(2.f * l1v[c], fmaf(p3, g3[o], fmaf(bw[o], t, bb[o])), LZ[ix]) : 0.f;
                LZ[ix] = lz; Pb3[ix] = g3[o] * lz;
            }
        }
    });
    ft_tr(W3, G.ld[2], G.inp[2], G.outp[2], V3, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; M2[ix] = v[j]; V2[ix] = v[j] * SG2[ix] * g2[r0 + j]; }
    });
    if constexpr (!KIN)
        ft_tr(W3, G.ld[2], G.inp[2], G.outp[2], Pb3, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) T2[(r0 + j) * 16 + c] = v[j];
        });
    __syncthreads();
    if constexpr (KIN)                 // (Pb3 was formed by the layer-3 epilogue above)
        ft_tr(W3, G.ld[2], G.inp[2], G.outp[2], Pb3, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) T2[(r0 + j) * 16 + c] = v[j];
        });
    // m1 = W2' v2; the reverse of tr = e . W1' v1 through layer 1
    ft_tr(W2, G.ld[1], G.inp[1], G.outp[1], V2, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j, ix = o * 16 + c;
            const float m1 = v[j], sg = SG1[ix], s = g1[o];
            M1[ix] = m1; V1[ix] = m1 * sg * s;
            if constexpr (!KIN) {
                const float vb = VB1[ix];
                CV1[ix] = cv[c] * (m1 * sg * s);
                Mb1[ix] = vb * sg * s; Hb1[ix] = vb * m1 * s * ff_dsig(sg); SB1[ix] = vb * m1 * sg;
            }
        }
    });
    __syncthreads();
    if constexpr (KIN) {               // w = c e + 2 l2 eJ (eJ = W1' v1), then v1-bar = W1 w where the plain sweep has c (W1 e)
        ft_tr(W1, G.ld[0], G.inp[0], G.outp[0], V1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; WV[ix] = fmaf(2.f * l2v[c], v[j], cv[c] * L.E[ix]); }
        });
        __syncthreads();
        ft_fwd(W1, G.ld[0], G.inp[0], G.outp[0], WV, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = r0 + j, ix = o * 16 + c;
                const float vb = v[j], m1 = M1[ix], sg = SG1[ix], s = g1[o];
                Mb1[ix] = vb * sg * s; Hb1[ix] = vb * m1 * s * ff_dsig(sg); SB1[ix] = vb * m1 * sg;
            }
        });
        __syncthreads();
    }
    // through layer 2 (trace), plus the primal's cotangent of h2
    ft_fwd(W2, G.ld[1], G.inp[1], G.outp[1], Mb1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j, ix = o * 16 + c;
            const float q = v[j], sg = SG2[ix], s = g2[o], m2 = M2[ix];
            const float hb = q * m2 * s * ff_dsig(sg) + T2[ix] * sg;
            Mb2[ix] = q * sg * s; Hb2[ix] = hb; Pb2[ix] = hb * s; SB2[ix] = q * m2 * sg + hb * P2[ix];
        }
    });
    __syncthreads();
    ft_fwd(W3, G.ld[2], G.inp[2], G.outp[2], Mb2, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; SB3[ix] = v[j] * L.E[ix] + LZ[ix] * P3[ix]; }
    });
    ft_tr(W2, G.ld[1], G.inp[1], G.outp[1], Pb2, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j, ix = o * 16 + c;
            const float hb = Hb1[ix] + v[j] * SG1[ix];
            Hb1[ix] = hb; Pb1[ix] = hb * g1[o]; SB1[ix] += hb * P1[ix];
        }
    });
    __syncthreads();
    ft_tr(W1, G.ld[0], G.inp[0], G.outp[0], Pb1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int r = r0 + j; if (r < D) yb[r * 16 + c] += v[j]; }
    });
    // parameter cotangents
    ft_wgrad(KIN ? V1 : CV1, KIN ? WV : L.E, Pb1, ZP, G.outp[0], G.inp[0], G.out[0], G.in[0], pacc + G.off[0], wave, lane);
    ft_wgrad(V2, Mb1, Pb2, X1, G.outp[1], G.inp[1], G.out[1], G.in[1], pacc + G.off[1], wave, lane);
    ft_wgrad(V3, Mb2, Pb3, X2, G.outp[2], G.inp[2], G.out[2], G.in[2], pacc + G.off[2], wave, lane);
    for (int q = tid; q < 2 * H + D; q += kFtThreads) {
        const int l = q < H ? 0 : (q < 2 * H ? 1 : 2), o = q - (l == 0 ? 0 : (l == 1 ? H : 2 * H));
        const float *pb = l == 0 ? Pb1 : (l == 1 ? Pb2 : Pb3), *beta = l == 0 ? Hb1 : (l == 1 ? Hb2 : LZ), *sb = l == 0 ? SB1 : (l == 1 ? SB2 : SB3);
        float a = 0.f, b = 0.f, s = 0.f;
        for (int k = 0; k < 16; ++k) { a += pb[o * 16 + k]; b += beta[o * 16 + k]; s += sb[o * 16 + k]; }
        const float gs = L.GT[(l == 0 ? 0 : (l == 1 ? HP : 2 * HP)) + o];
        float* pv = pacc + G.off[l] + G.in[l] * G.out[l];
        const int out = G.out[l];
        pv[o] += a;
        pv[out + o] += b * t;
        pv[2 * out + o] += b;
        pv[3 * out + o] += s * ff_dsig(gs) * t;
    }
    __syncthreads();
}

template <bool KIN>
__global__ __launch_bounds__(kFtThreads) void rnde_ffjordt_reverse_kernel(const FtRevParams Q) {
    extern __shared__ float ft_smem[];
    const FtGeo& G = Q.G;
    const int tile = blockIdx.x, tid = threadIdx.x, D = G.D, R = D + (KIN ? 3 : 1), Bp = Q.Bp, col0 = tile * 16, nel = R * 16;
    const FtLds L = ft_lds(G, ft_smem);
    ft_load_params(G, Q.p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        L.E[idx] = (r < D && col < Q.B) ? Q.e[(size_t)col * D + r] : 0.f;
        L.X[idx] = 0.f;
    }
    float* ws = Q.ws + (size_t)tile * ft_rev_ws_floats(G, KIN);
    const size_t RS = (size_t)R * 16;
    auto Ys = [&](int s) { return ws + (size_t)s * RS; };
    auto Ks = [&](int s) { return ws + (size_t)(7 + s) * RS; };
    auto Kb = [&](int s) { return ws + (size_t)(14 + s) * RS; };
    float *UB = ws + 21 * RS, *UBn = ws + 22 * RS, *Yb = ws + 23 * RS, *V = ws + 24 * RS;
    float* pacc = Q.pacc + (size_t)tile * G.P;
    for (int q = tid; q < G.P; q += kFtThreads) pacc[q] = 0.f;
    const size_t RB = (size_t)R * Bp;
    for (int idx = tid; idx < nel; idx += kFtThreads) {     // logpx = sum -(log 2 pi + z^2) / 2 - l
        const int r = idx >> 4, c = idx & 15, col = col0 + c;
        float v = 0.f;
        if (col < Q.B) {
            const float g = Q.logpx_bar[col];
            v = r < D ? -g * Q.tape[(size_t)Q.n_acc * RB + (size_t)r * Bp + col] : -g;
            if constexpr (KIN)
                if (r > D) v = Q.reg_bar ? Q.reg_bar[(size_t)(r - D - 1) * Q.B + col] : 0.f;
        }
        UB[idx] = v;
    }
    __syncthreads();
    const double N = (double)R * (double)Q.B;
    for (int n = Q.n_acc - 1; n >= 0; --n) {
        const FfStepRec st = Q.rec[n];
        const float t = st.t, dt = st.dt;
        const float* U = Q.tape + (size_t)n * RB + col0;
        // ---- recompute the stages ----
        for (int s = 0; s < 7; ++s) {
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                float acc = 0.f;
                for (int j = 0; j < s; ++j) acc = fmaf(tsA_rt(s, j), Ks(j)[idx], acc);
                const float y = U[(size_t)r * Bp + c] + dt * acc;
                Ys(s)[idx] = y;
                if (r < D) L.X[idx] = y;
            }
            ft_eval<KIN>(G, L, t + kTsC[s] * dt, Ks(s), 16, 0, 1.f, -1.f, nullptr, tid);
        }
        for (int idx = tid; idx < nel; idx += kFtThreads) {
            for (int s = 0; s < 7; ++s) Kb(s)[idx] = 0.f;
            UBn[idx] = 0.f;
            Yb[idx] = UB[idx];                                // cotangent of unew = stage-7 input
        }
        // ---- A: reverse of the error estimate (the saved value EEst * dt; rnde_bffjord.h) ----
        if (st.svb != 0.f && st.eest > 0.f) {
            const float coef = (float)(((double)st.svb * (double)dt) / (N * (double)st.eest));
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
            ft_vjp<KIN>(G, L, t + kTsC[s] * dt, Ys(s), Kb(s), Yb, V, pacc, tid);
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float y = Yb[idx];
                UBn[idx] += y;
                for (int j = 0; j < s; ++j) Kb(j)[idx] += dt * tsA_rt(s, j) * y;
            }
            __syncthreads();
        }
        for (int idx = tid; idx < nel; idx += kFtThreads) UB[idx] = UBn[idx];
        __syncthreads();
    }
    if (Q.x_bar)
        for (int idx = tid; idx < nel; idx += kFtThreads) {
            const int r = idx >> 4, col = col0 + (idx & 15);
            if (r < D && col < Q.B) Q.x_bar[(size_t)col * D + r] = UB[idx];
        }
}

// p_bar[q] = sum over tiles of pacc[tile][q], in tile order, carried in double
__global__ __launch_bounds__(256) void rnde_ffjordt_reduce_kernel(const float* __restrict__ pacc, int P, int ntiles, float* __restrict__ p_bar) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P) return;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s += (double)pacc[(size_t)t * P + q];
    p_bar[q] = (float)s;
}

}  // namespace rnde
