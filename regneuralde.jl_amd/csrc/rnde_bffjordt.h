// rnde_bffjordt.h -- the reverse of the ConcatSquash dynamics on the tile layout: FtDyn::vjp, one stage's second-order VJP as
// rnde_tile_driver.h's reverse sweep calls it, and what it shares with the Dense-chain dynamics (ft_wgrad).
//
// The second-order VJP of a stage needs some 27 per-column vectors; next to the resident weights they do not fit in LDS at the tabular
// widths, so they live in a per-tile global buffer (written and read by the same workgroup, L2-resident); no private scratch.  Every
// product, the weight cotangents included (outer products over the tile's 16 columns, k = 2 x 16), runs on the matrix cores.
//
// Kinetic variant (KIN; the arithmetic of rnde_bffjord.h): the stage cotangent is (lz, ll, l1, l2) over R = D + 3 rows.  The cotangent of f,
// lz + 2 l1 f, is formed in the epilogue of the layer-3 product; w = -ll e + 2 l2 eJ needs eJ = W1' v1, one more transposed product once v1
// is known, and W1 w replaces c (W1 e).  Both are two more vector slots of the per-tile global buffer: no LDS beyond the plain kernel's.
#pragma once
#include "rnde_bffjord.h"      // ff_dsig
#include "rnde_ffjordt.h"

namespace rnde {

constexpr int kFtVjpVecs = 27;
constexpr int kFtVjpVecsKin = 28;      // + w (the cotangent of eJ)

__host__ __device__ inline size_t FtDyn::rev_ws_floats(const FtGeo& G, bool kin) {
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
// Returns this thread's share of <dF/dt, lam> summed over the tile's columns (the tracked sweep's time cotangent): h = p sig(gw t) + bw t + bb,
// so wherever t X goes to gw-bar, gw X goes to the sum (formed ahead of the product with t: t = 0 occurs), and <bw, bb-bar> with it.
template <bool KIN>
__device__ __forceinline__ float FtDyn::vjp(const FtGeo& G, const FtLds& L, float t, const float* z, const float* kb, float* yb, float* V, float* pacc, int tid, float*) {
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
    float tsum = 0.f;
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
        tsum = fmaf(ft_vec(G, L.W, l, 3)[o], s * ff_dsig(gs), fmaf(ft_vec(G, L.W, l, 1)[o], b, tsum));
    }
    __syncthreads();
    return tsum;
}

}  // namespace rnde
