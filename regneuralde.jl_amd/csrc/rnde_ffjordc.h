// rnde_ffjordc.h -- TrackedFFJORD's default dynamics (ffjord.jl:21-27: Tracker.forward(z -> m(z, t), z) and back(e)) for a chain of Dense
// layers, plain (Chain) or time dependent (TDChain: t appended to every layer's input), on the tile layout of rnde_ffjordt.h
// (FcDyn; rnde_ffjord_create_chain, engine 2).  The solve, the reverse sweep and the feval kernel are rnde_tile_driver.h's.
//
// Dynamics, y_0 = z:   a_l = W_l y_{l-1} + wt_l t + b_l,   y_l = phi_l(a_l),   f = y_n,   d_l = phi_l' taken from y_l (act_dy)
//     v_n = d_n .* e,   m_l = W_{l+1}' v_{l+1} (the z columns only),   v_l = d_l .* m_l,   eJ = W_1' v_1,   F = [f; -e . eJ]
// KIN: F = [f; -e . eJ; sum f^2; sum eJ^2] (ffjord.jl:53-66).  The exact trace (sample, feval exact) is D passes of the same VJP with
// unit probes, as the reference's jacobian_fn.
//
// Geometry: rnde_ffjordt.h's.  One workgroup of four waves per 16 batch columns; the padded weights resident in LDS as Wl[in][ld]
// (ld = outp + 1), the t column and the bias as two per-output vectors beside them (the t column is an epilogue term, `in` is not padded
// to in + 1); activations [feature][16]; layer products through ft_fwd / ft_tr.  Every layer's output stays in LDS for the VJP (d_l is read
// from it), two more vectors carry v_l down the chain.  Limits come from bytes: FcDyn::lds_floats(G) * 4 <= 160 KB, checked at create.
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
struct FcLds {
    float* W;
    float *X, *E;                      // [DP][16]: the chain's input, the probe
    float* Y;                          // every layer's output, layer l at Y + yoff[l] ([outp_l][16], padded rows zero)
    float *V0, *V1;                    // [MP][16]: v_l going down the chain
    float* red;                        // 128 floats (the meeting keeps doubles at red + 64)
};

// The Dense-chain dynamics as the tile driver sees them (the policy's contract: rnde_tile_driver.h).
struct FcDyn {
    using Geo = FcGeo;
    using Lds = FcLds;
    static constexpr int kAug = 1;                                                       // [z; l]: the log-density row
    static constexpr bool kProbe = true, kDensity = true, kSpan = false, kVjpKdot = false;
    // LDS floats of the solve / feval / reverse kernels: parameters, X, E, every layer's output, two VJP vectors, reduction scratch
    __host__ __device__ static int lds_floats(const FcGeo& G) { return ft_align4(G.wfloats) + 2 * G.DP * 16 + G.yfloats + 2 * G.MP * 16 + 128; }
    __host__ __device__ static size_t scratch_floats(const FcGeo&) { return 0; }                          // (the exact trace needs none)
    __host__ __device__ static size_t rev_ws_floats(const FcGeo& G, bool kin = false);                    // (rnde_bffjordc.h)
    __device__ static FcLds lds(const FcGeo& G, float* smem) {
        FcLds L;
        L.W = smem;
        float* b = smem + ft_align4(G.wfloats);
        L.X = b; b += G.DP * 16; L.E = b; b += G.DP * 16;
        L.Y = b; b += G.yfloats;
        L.V0 = b; b += G.MP * 16; L.V1 = b; b += G.MP * 16;
        L.red = b;
        return L;
    }
    // parameters into LDS, zero-padded (every thread of the workgroup); no barrier: eval opens with one
    __device__ static void load_params(const FcGeo& G, const float* __restrict__ p, float* W, int tid) {
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
    template <bool KIN>
    __device__ static void eval(const FcGeo& G, const FcLds& L, float t, float* kout, int ks, int exact, float fsign, float tsign, float* scratch, int tid);
    template <bool KIN>
    __device__ static float vjp(const FcGeo& G, const FcLds& L, float t, const float* z, const float* kb, float* yb, float* V, float* pacc, int tid, float* kdot);      // (rnde_bffjordc.h)
};

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

// One evaluation of the augmented right-hand side for the 16 columns of a tile (the policy's eval).  exact: D unit-probe passes; no scratch.
template <bool KIN>
__device__ __forceinline__ void FcDyn::eval(const FcGeo& G, const FcLds& L, float t, float* kout, int ks, int exact, float fsign, float tsign, float*, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, n = G.n;
    __syncthreads();                   // the contract's barrier ahead of the first read of L.X (and of the parameters load_params wrote)
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

}  // namespace rnde
