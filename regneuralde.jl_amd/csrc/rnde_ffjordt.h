// rnde_ffjordt.h -- the tile layout of TrackedFFJORD and its ConcatSquash dynamics (FtDyn; rnde_ffjord_create_tiled, engine 1): the dynamics
// of rnde_ffjord.h at widths the one-workgroup engine does not serve (the tabular experiment's 43 -> 100), with the layer products on the
// matrix cores.  The solve, the reverse sweep and the feval kernel that run these dynamics are rnde_tile_driver.h's; what is shared with the
// Dense-chain dynamics (rnde_ffjordc.h) is here: the kFt* constants, ft_pad16, ft_align4, ft_fwd, ft_tr, ft_colsum.
//
// Geometry (rnde_chainmw.h's layout): one workgroup of four waves per 16 batch columns (a tile).  The padded parameters stay resident in LDS,
// each layer's weights as Wl[in][ld] (ld = outp + 1: the transposed products read rows, the forward products columns, neither conflicts),
// zero outside the layer.  Activations live in LDS as [feature][16 columns]; a layer product is v_mfma_f32_16x16x4_f32 (exact fp32
// products), wave w owning output tiles w, w + 4, ...; its epilogue applies gate / shift / softplus in registers and writes the next
// activation.  Padded feature rows are written as zero by every epilogue, padded columns of a partial last tile carry zero probes and zero
// cotangents and are left out of every norm.
//
// Exact trace (sample, feval exact): with a1 = sig(h1) .* g1, a2 = sig(h2) .* g2,
//     tr J = a2' (W2 .* M') a1,   M(t) = W1 diag(g3(t)) W3   (H x H)
// Each tile forms QT = (W2 .* M')' once per evaluation on the matrix cores into a tile-private global buffer (the driver's scratch); each
// column then costs one H x H product.
//
// Kinetic variant (template parameter KIN; rnde_ffjord.h): R = D + 3 rows, the two regulariser rates sum f^2 and sum eJ^2 formed where the
// trace is formed -- per-lane partials in the epilogues of the layer-3 product and of the last transposed product, then the same per-column
// reduction.  No LDS beyond the plain kernels' (135 KB at (43, 100)), so the limits are the plain ones: in_dims <= 64, hidden <= 112.
#pragma once
#include "rnde_chainmw.h"     // rnde_meet.h, kMwMeetMax, mfma16
#include "rnde_ffjord.h"

namespace rnde {

constexpr int kFtWaves = 4;
constexpr int kFtThreads = 64 * kFtWaves;
constexpr int kFtMaxD = 64;            // the tiled engine's width limit (LDS: weights + activations of the solve within 160 KB)
constexpr int kFtMaxH = 112;
constexpr int kFtLdsBytes = 160 * 1024;
constexpr int kFtMaxAttempts = 8000;   // two initial meetings + one per attempt, below kMeetRows (rnde_meet.h)

struct FtGeo {
    int D, H, P, DP, HP;
    int off[3], in[3], out[3];         // parameter offsets and widths (as FfGeo)
    int inp[3], outp[3], ld[3];        // padded widths (16), LDS row stride of Wl
    int woff[3], voff[3];              // LDS offsets (floats) of Wl and of the four vectors b, bw, bb, gw (outp each)
    int wfloats;                       // LDS floats of the parameters
};

__host__ __device__ inline int ft_pad16(int n) { return (n + 15) / 16 * 16; }
__host__ inline FtGeo ft_geo(int D, int H) {
    FtGeo G;
    const FfGeo F = ff_geo(D, H);
    G.D = D; G.H = H; G.P = F.P; G.DP = ft_pad16(D); G.HP = ft_pad16(H);
    int o = 0;
    for (int l = 0; l < 3; ++l) {
        G.off[l] = F.off[l]; G.in[l] = F.in[l]; G.out[l] = F.out[l];
        G.inp[l] = ft_pad16(F.in[l]); G.outp[l] = ft_pad16(F.out[l]); G.ld[l] = G.outp[l] + 1;
        G.woff[l] = o; o += G.inp[l] * G.ld[l];
    }
    for (int l = 0; l < 3; ++l) { G.voff[l] = o; o += 4 * G.outp[l]; }
    G.wfloats = o;
    return G;
}
__host__ __device__ inline int ft_gt_floats(const FtGeo& G) { return 2 * G.HP + G.DP; }
__host__ __device__ inline int ft_align4(int n) { return (n + 3) & ~3; }

struct FtLds {
    float* W;                          // parameters (ft_geo layout)
    float* GT;                         // gates at the evaluation time: g1 [HP], g2 [HP], g3 [DP] (zero on padded rows)
    float *X, *E;                      // [DP][16]: the layer-1 input / Hutchinson scratch, the probe
    float *S1, *A1, *S2, *A2;          // [HP][16]: softplus(h_l), sig(h_l) .* g_l (then the VJP's v2, v1 in S1, S2)
    float* red;                        // 64 floats (+ 64 for the meeting)
};

// The ConcatSquash dynamics as the tile driver sees them (the policy's contract: rnde_tile_driver.h).
struct FtDyn {
    using Geo = FtGeo;
    using Lds = FtLds;
    static constexpr int kAug = 1;                                                       // [z; l]: the log-density row
    static constexpr bool kProbe = true, kDensity = true, kSpan = false, kVjpKdot = false;
    // LDS floats of the solve / feval / reverse kernels: parameters, gates, six activation buffers, reduction scratch
    __host__ __device__ static int lds_floats(const FtGeo& G) { return ft_align4(G.wfloats) + ft_align4(ft_gt_floats(G)) + (2 * G.DP + 4 * G.HP) * 16 + 128; }
    __host__ __device__ static size_t scratch_floats(const FtGeo& G) { return (size_t)G.HP * G.HP; }      // QT of the exact trace
    __host__ __device__ static size_t rev_ws_floats(const FtGeo& G, bool kin = false);                    // (rnde_bffjordt.h)
    __device__ static FtLds lds(const FtGeo& G, float* smem) {
        FtLds L;
        L.W = smem; L.GT = smem + ft_align4(G.wfloats);
        float* b = L.GT + ft_align4(ft_gt_floats(G));      // (the meeting keeps doubles at red + 64: 8-byte aligned)
        L.X = b; b += G.DP * 16; L.E = b; b += G.DP * 16;
        L.S1 = b; b += G.HP * 16; L.A1 = b; b += G.HP * 16; L.S2 = b; b += G.HP * 16; L.A2 = b; b += G.HP * 16;
        L.red = b;
        return L;
    }
    // parameters into LDS, zero-padded (every thread of the workgroup); ends behind a barrier: eval and vjp open with ft_gates, which reads
    // gate_W from LDS ahead of their first barrier
    __device__ static void load_params(const FtGeo& G, const float* __restrict__ p, float* W, int tid) {
        for (int l = 0; l < 3; ++l) {
            const int ld = G.ld[l], in = G.in[l], out = G.out[l], n = G.inp[l] * ld;
            float* w = W + G.woff[l];
            for (int idx = tid; idx < n; idx += kFtThreads) {
                const int i = idx / ld, o = idx - i * ld;
                w[idx] = (i < in && o < out) ? p[G.off[l] + i * out + o] : 0.f;
            }
            float* v = W + G.voff[l];
            for (int idx = tid; idx < 4 * G.outp[l]; idx += kFtThreads) {
                const int k = idx / G.outp[l], o = idx - k * G.outp[l];
                v[idx] = o < out ? p[G.off[l] + in * out + k * out + o] : 0.f;
            }
        }
        __syncthreads();
    }
    template <bool KIN>
    __device__ static void eval(const FtGeo& G, const FtLds& L, float t, float* kout, int ks, int exact, float fsign, float tsign, float* QT, int tid);
    template <bool KIN>
    __device__ static float vjp(const FtGeo& G, const FtLds& L, float t, const float* z, const float* kb, float* yb, float* V, float* pacc, int tid, float* kdot);      // (rnde_bffjordt.h)
};
__device__ __forceinline__ const float* ft_vec(const FtGeo& G, const float* W, int l, int k) { return W + G.voff[l] + k * G.outp[l]; }

__device__ inline void ft_gates(const FtGeo& G, const float* W, float* GT, float t, int tid) {
    const int n = ft_gt_floats(G);
    for (int idx = tid; idx < n; idx += kFtThreads) {
        int l, o;
        if (idx < G.HP) { l = 0; o = idx; } else if (idx < 2 * G.HP) { l = 1; o = idx - G.HP; } else { l = 2; o = idx - 2 * G.HP; }
        GT[idx] = o < G.out[l] ? ff_sig(ft_vec(G, W, l, 3)[o] * t) : 0.f;
    }
}

// Y = W_l X (forward product): output tiles over outp, k over inp; X [inp][16].  epi(row0, v): rows row0 + j (j < 4), column lane & 15.
template <class Epi>
__device__ __forceinline__ void ft_fwd(const float* Wl, int ld, int inp, int outp, const float* X, int wave, int lane, Epi&& epi) {
    const int c = lane & 15, g = lane >> 4;
    for (int mo = wave; mo < (outp >> 4); mo += kFtWaves) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const float* wp = Wl + 16 * mo + c + g * ld;
        const float* xp = X + g * 16 + c;
        for (int k = 0; k < inp; k += 8) {
            a0 = mfma16(wp[k * ld], xp[k * 16], a0);
            a1 = mfma16(wp[(k + 4) * ld], xp[(k + 4) * 16], a1);
        }
        epi(16 * mo + 4 * g, a0 + a1);
    }
}
// Y = W_l' X (transposed product): output tiles over inp, k over outp; X [outp][16]
template <class Epi>
__device__ __forceinline__ void ft_tr(const float* Wl, int ld, int inp, int outp, const float* X, int wave, int lane, Epi&& epi) {
    const int c = lane & 15, g = lane >> 4;
    for (int mi = wave; mi < (inp >> 4); mi += kFtWaves) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const float* wp = Wl + (16 * mi + c) * ld + g;
        const float* xp = X + g * 16 + c;
        for (int k = 0; k < outp; k += 8) {
            a0 = mfma16(wp[k], xp[k * 16], a0);
            a1 = mfma16(wp[k + 4], xp[(k + 4) * 16], a1);
        }
        epi(16 * mi + 4 * g, a0 + a1);
    }
}

// Per-column sum over rows of a product formed in registers (every wave's lanes hold partials of column lane & 15): butterfly inside the
// wave, then the waves in order.  Returns the sum on threads tid < 16 (column tid); ends behind a barrier.
__device__ __forceinline__ float ft_colsum(float v, float* red, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < 16) red[wave * 16 + lane] = v;
    __syncthreads();
    float s = 0.f;
    if (tid < 16) s = ((red[tid] + red[16 + tid]) + red[32 + tid]) + red[48 + tid];
    __syncthreads();
    return s;
}

// One evaluation of the augmented right-hand side for the 16 columns of a tile (the policy's eval).  exact: the closed-form trace (QT: this
// tile's H x H buffer).  The barrier behind ft_gates is the one the contract asks for ahead of the first read of L.X.
template <bool KIN>
__device__ __forceinline__ void FtDyn::eval(const FtGeo& G, const FtLds& L, float t, float* kout, int ks, int exact, float fsign, float tsign, float* QT, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, H = G.H, HP = G.HP;
    const float *W1 = L.W + G.woff[0], *W2 = L.W + G.woff[1], *W3 = L.W + G.woff[2];
    const float *g1 = L.GT, *g2 = L.GT + HP, *g3 = L.GT + 2 * HP;
    ft_gates(G, L.W, L.GT, t, tid);
    __syncthreads();
    if (exact) {   // QT[j][k] = W2[k][j] M[j][k], M[j][k] = sum_i W1[j][i] g3_i W3[i][k]
        const int g = lane >> 4, nt = HP >> 4, ld1 = G.ld[0], ld2 = G.ld[1], ld3 = G.ld[2];
        for (int tt = wave; tt < nt * nt; tt += kFtWaves) {
            const int mj = tt / nt, mk = tt - mj * nt;
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            for (int i = 0; i < G.DP; i += 8) {
                a0 = mfma16(W1[(i + g) * ld1 + 16 * mj + c], g3[i + g] * W3[(16 * mk + c) * ld3 + i + g], a0);
                a1 = mfma16(W1[(i + 4 + g) * ld1 + 16 * mj + c], g3[i + 4 + g] * W3[(16 * mk + c) * ld3 + i + 4 + g], a1);
            }
            const f32x4 m = a0 + a1;
            const int k = 16 * mk + c;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = 16 * mj + 4 * g + jj;
                QT[(size_t)j * HP + k] = W2[j * ld2 + k] * m[jj];
            }
        }
    }
    // layer 1 -> S1, A1
    ft_fwd(W1, G.ld[0], G.inp[0], G.outp[0], L.X, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 0, 0), *bw = ft_vec(G, L.W, 0, 1), *bb = ft_vec(G, L.W, 0, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j;
            float s = 0.f, a = 0.f;
            if (o < H) { const float h = fmaf(v[j] + b[o], g1[o], fmaf(bw[o], t, bb[o])); s = ff_softplus(h); a = ff_sig(h) * g1[o]; }
            L.S1[o * 16 + c] = s; L.A1[o * 16 + c] = a;
        }
    });
    __syncthreads();
    // layer 2 -> S2, A2
    ft_fwd(W2, G.ld[1], G.inp[1], G.outp[1], L.S1, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 1, 0), *bw = ft_vec(G, L.W, 1, 1), *bb = ft_vec(G, L.W, 1, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j;
            float s = 0.f, a = 0.f;
            if (o < H) { const float h = fmaf(v[j] + b[o], g2[o], fmaf(bw[o], t, bb[o])); s = ff_softplus(h); a = ff_sig(h) * g2[o]; }
            L.S2[o * 16 + c] = s; L.A2[o * 16 + c] = a;
        }
    });
    __syncthreads();
    // layer 3 -> f;  Hutchinson: X <- g3 .* e;  exact: tr = a2 . (Q a1)
    float pke = 0.f, pjn = 0.f;
    ft_fwd(W3, G.ld[2], G.inp[2], G.outp[2], L.S2, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 2, 0), *bw = ft_vec(G, L.W, 2, 1), *bb = ft_vec(G, L.W, 2, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j;
            if (o < D) {
                const float f = fmaf(v[j] + b[o], g3[o], fmaf(bw[o], t, bb[o]));
                kout[(size_t)o * ks + c] = fsign * f;
                if constexpr (KIN) pke = fmaf(f, f, pke);
            }
        }
    });
    float part = 0.f;
    if (exact) {
        ft_fwd(QT, HP, HP, HP, L.A1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) part = fmaf(L.A2[(r0 + j) * 16 + c], v[j], part);
        });
    } else {
        for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) L.X[idx] = g3[idx >> 4] * L.E[idx];
        __syncthreads();
        // v2 = a2 .* W3' (g3 .* e) -> S1
        ft_tr(W3, G.ld[2], G.inp[2], G.outp[2], L.X, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int o = r0 + j; L.S1[o * 16 + c] = v[j] * L.A2[o * 16 + c]; }
        });
        __syncthreads();
        // v1 = a1 .* W2' v2 -> S2
        ft_tr(W2, G.ld[1], G.inp[1], G.outp[1], L.S1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int o = r0 + j; L.S2[o * 16 + c] = v[j] * L.A1[o * 16 + c]; }
        });
        __syncthreads();
        // tr = e . W1' v1
        ft_tr(W1, G.ld[0], G.inp[0], G.outp[0], L.S2, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                part = fmaf(L.E[(r0 + j) * 16 + c], v[j], part);
                if constexpr (KIN) pjn = fmaf(v[j], v[j], pjn);      // (rows >= D: W1's padded rows are zero)
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

}  // namespace rnde
