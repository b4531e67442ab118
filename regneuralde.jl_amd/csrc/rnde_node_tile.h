// rnde_node_tile.h -- TrackedNeuralODE over a Dense chain on the tile layout of rnde_ffjordt.h (rnde_node_create_tiled, engine 4): NtDyn,
// the third dynamics of the tile driver (rnde_tile_driver.h has the solve, the reverse sweeps, the feval kernel and the policy's contract).
// The right-hand side is the chain itself, f(u, t) = y_n, with no trace row and no probe.  What TrackedFFJORD's chain dynamics built serves
// here unchanged: the geometry (FcGeo, fc_geo), the parameter load (FcDyn::load_params), the chain evaluation (fc_chain) and the layer
// products (ft_fwd / ft_tr).
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
// One stage's VJP, cotangent kb of f(y, t), notation of rnde_ffjordc.h (d_l = phi_l' taken from the layer's output):
//     v_n = d_n .* kb,   v_l = d_l .* W_{l+1}' v_{l+1},   yb += W_1' v_1
//     W_l-bar += v_l y_{l-1}',   wt_l-bar += t sum_c v_l,   b_l-bar += sum_c v_l        (outer products over the tile's 16 columns)
// The transposed products are ft_tr, the outer products one v_mfma_f32_16x16x4_f32 chain per 16 x 16 block of W_l (k = the 16 columns).
// Every entry of pacc has one owner lane for the whole sweep.
#pragma once
#include "rnde_ffjordc.h"          // FcGeo, fc_geo, FcDyn::load_params, fc_chain; rnde_ffjordt.h

namespace rnde {

struct NtLds {
    float* W;
    float* X;                          // [DP][16]: the chain's input (padded rows zero)
    float* Y;                          // every layer's output, layer l at Y + yoff[l] ([outp_l][16], padded rows zero)
    float *V0, *V1;                    // [MP][16]: v_l going down the chain (reverse sweep)
    float* red;                        // 128 floats (the meeting keeps doubles at red + 64)
};

// dW[o][i] += sum_c A[o][c] Bm[i][c] (both [feature][16]) into pw[i * out + o]; output blocks dealt to the waves
__device__ __forceinline__ void nt_wgrad(const float* A, const float* Bm, int outp, int inp, int out, int in, float* pw, int wave, int lane) {
    const int c = lane & 15, g = lane >> 4, nti = inp >> 4, nt = (outp >> 4) * nti;
    for (int tt = wave; tt < nt; tt += kFtWaves) {
        const int mo = tt / nti, mi = tt - mo * nti;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int ao = (16 * mo + c) * 16 + g, bo = (16 * mi + c) * 16 + g;
#pragma unroll
        for (int kc = 0; kc < 16; kc += 4) acc = mfma16(A[ao + kc], Bm[bo + kc], acc);
        const int i = 16 * mi + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = 16 * mo + 4 * g + j;
            if (o < out && i < in) pw[(size_t)i * out + o] += acc[j];
        }
    }
}

// yb[0:D] += (df/dy)' kb and pacc += (df/dp)' kb at the stage input y ([D][16]) for the tile's 16 columns.  Every thread of the workgroup
// calls it; ends behind a barrier.  TAU (the tracked sweep): returns the calling thread's share of <df/dt, kb> over the tile's columns,
// sum_l sum_o wt_l[o] sum_c v_l[o][c], from the per-output column sums formed for the bias anyway (zero for a plain Chain), and adds its share
// of <f(y, t), kb> to kdot: the chain's last output, recomputed here in LDS, is f itself, and kb is read for v_n anyway, so the sum
// <k_s, k_s-bar> of the dt cotangent costs no pass over global memory.  Without TAU the function returns 0 and forms neither.
template <bool TAU>
__device__ __forceinline__ float nt_vjp(const FcGeo& G, const NtLds& L, float t, const float* y, const float* kb, float* yb, float* pacc, int tid,
                                        float* kdot) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, n = G.n;
    float tsum = 0.f;
    for (int idx = tid; idx < D * 16; idx += kFtThreads) L.X[idx] = y[idx];      // (rows >= D of L.X are zero and stay so)
    __syncthreads();
    fc_chain(G, L.W, L.X, L.Y, t, wave, lane, [](int, int, float) {});
    float *va = L.V0, *vb = L.V1;
    {
        const float* yn = L.Y + G.yoff[n - 1];
        const int code = G.act[n - 1];
        if constexpr (TAU) {
            float kd = 0.f;
            for (int idx = tid; idx < G.outp[n - 1] * 16; idx += kFtThreads) {
                float v = 0.f;
                if ((idx >> 4) < D) { const float f = yn[idx], b = kb[idx]; v = act_dy(code, f) * b; kd = fmaf(f, b, kd); }
                va[idx] = v;
            }
            *kdot += kd;
        } else {
            for (int idx = tid; idx < G.outp[n - 1] * 16; idx += kFtThreads) va[idx] = (idx >> 4) < D ? act_dy(code, yn[idx]) * kb[idx] : 0.f;
        }
    }
    __syncthreads();
    for (int l = n - 1; l >= 0; --l) {      // layer l (0-based): input y_{l-1} (L.X for l = 0), cotangent of its pre-activation in va
        const int in = G.dims[l], out = G.dims[l + 1];
        const float* yin = l ? L.Y + G.yoff[l - 1] : L.X;
        float* pl = pacc + G.off[l];
        nt_wgrad(va, yin, G.outp[l], G.inp[l], out, in, pl, wave, lane);
        for (int o = tid; o < out; o += kFtThreads) {
            float s = 0.f;
            for (int k = 0; k < 16; ++k) s += va[o * 16 + k];
            if (G.td) {
                pl[in * out + o] += t * s;
                if constexpr (TAU) tsum = fmaf(L.W[G.voff[l] + o], s, tsum);
            }
            pl[(in + G.td) * out + o] += s;
        }
        if (l > 0) {
            const int code = G.act[l - 1];
            ft_tr(L.W + G.woff[l], G.ld[l], G.inp[l], G.outp[l], va, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; vb[ix] = v[j] * act_dy(code, yin[ix]); }
            });
        } else {
            ft_tr(L.W + G.woff[0], G.ld[0], G.inp[0], G.outp[0], va, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int r = r0 + j; if (r < D) yb[r * 16 + c] += v[j]; }
            });
        }
        __syncthreads();
        float* s = va; va = vb; vb = s;
    }
    return tsum;
}

// The Dense chain as the tile driver sees it (the policy's contract: rnde_tile_driver.h).
struct NtDyn {
    using Geo = FcGeo;
    using Lds = NtLds;
    static constexpr int kAug = 0;                                                       // the state is u itself
    static constexpr bool kProbe = false, kDensity = false, kSpan = true, kVjpKdot = true;
    __host__ __device__ static int lds_floats(const FcGeo& G) { return ft_align4(G.wfloats) + G.DP * 16 + G.yfloats + 2 * G.MP * 16 + 128; }
    __host__ __device__ static size_t scratch_floats(const FcGeo&) { return 0; }
    // the reverse sweep's per-tile global workspace: stage inputs, stage values, stage cotangents (7 each), ub, ub-next, yb (no vector slots)
    __host__ __device__ static size_t rev_ws_floats(const FcGeo& G, bool = false) { return (size_t)24 * G.D * 16; }
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
    __device__ static __forceinline__ void load_params(const FcGeo& G, const float* __restrict__ p, float* W, int tid) { FcDyn::load_params(G, p, W, tid); }
    // kout[o * ks + c] = f_o(X, t) for o < D.  Opens with the barrier ahead of the first read of L.X (and of the parameters), ends behind one.
    template <bool KIN>
    __device__ static __forceinline__ void eval(const FcGeo& G, const NtLds& L, float t, float* kout, int ks, int, float, float, float*, int tid) {
        __syncthreads();
        fc_chain(G, L.W, L.X, L.Y, t, tid >> 6, tid & 63, [&](int o, int cc, float f) { kout[(size_t)o * ks + cc] = f; });
    }
    // (kdot != NULL is the tracked sweep: the time share and <f, kb> are formed there alone)
    template <bool KIN>
    __device__ static __forceinline__ float vjp(const FcGeo& G, const NtLds& L, float t, const float* z, const float* kb, float* yb, float*, float* pacc,
                                                int tid, float* kdot) {
        return kdot ? nt_vjp<true>(G, L, t, z, kb, yb, pacc, tid, kdot) : nt_vjp<false>(G, L, t, z, kb, yb, pacc, tid, nullptr);
    }
};

}  // namespace rnde
