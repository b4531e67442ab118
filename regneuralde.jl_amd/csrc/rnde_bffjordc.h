// rnde_bffjordc.h -- the reverse of the Dense-chain dynamics on the tile layout: FcDyn::vjp, one stage's second-order VJP as
// rnde_tile_driver.h's reverse sweep calls it.
//
// One stage, cotangent (lz, ll, l1, l2) of F = [f; -e . eJ; sum f^2; sum eJ^2] (plain sweep: l1 = l2 = 0), notation of rnde_ffjordc.h:
//     lf = lz + 2 l1 f,   w = -ll e + 2 l2 eJ                                   (the cotangents of f and of eJ)
//     v1-bar = W_1 w,  W_1-bar += v_1 w'                                         (eJ = W_1' v_1)
//     up the chain:  m_l-bar = d_l .* v_l-bar,  d_l-bar = m_l .* v_l-bar,  v_{l+1}-bar = W_{l+1} m_l-bar,  W_{l+1}-bar += v_{l+1} m_l-bar',
//                    d_n-bar = e .* v_n-bar
//     primal walk, y_n-bar = lf:  a_l-bar = y_l-bar .* d_l + d_l-bar .* phi_l''(y_l),  y_{l-1}-bar = W_l' a_l-bar,
//                    W_l-bar += a_l-bar y_{l-1}',  b_l-bar += a_l-bar,  wt_l-bar += t a_l-bar,  z-bar = y_0-bar
// phi'' is taken from the layer's output like phi' (act_d2y).
//
// The 5 n + 4 per-column vectors of the second-order reverse live in the tile's global buffer (written and read by the same workgroup,
// L2-resident), as in rnde_bffjordt.h; no private scratch.  Every product runs on the matrix cores, the weight cotangents through ft_wgrad
// (both outer products of a layer in one pass).
#pragma once
#include "rnde_bffjordt.h"     // ft_wgrad
#include "rnde_ffjordc.h"

namespace rnde {

__host__ __device__ inline int fc_vjp_vecs(const FcGeo& G) { return 5 * G.n + 4; }
__host__ __device__ inline size_t FcDyn::rev_ws_floats(const FcGeo& G, bool kin) {
    const int R = G.D + (kin ? 3 : 1);
    return (size_t)24 * R * 16 + (size_t)fc_vjp_vecs(G) * G.MP * 16;
}

// yb[0:D] += (dF/dz)' lam and pacc += (dF/dp)' lam for the tile's 16 columns.  z: the stage input ([R][16]), kb: its cotangent lam
// ([R][16]), yb: [R][16], V: the tile's vector slots.  Ends behind a barrier.
// Returns this thread's share of <dF/dt, lam> summed over the tile's columns (the tracked sweep's time cotangent): a_l = W_l y + wt_l t + b_l,
// so it is sum_l <wt_l, a_l-bar summed over the columns>, first- and second-order parts alike; zero for a plain Chain.
template <bool KIN>
__device__ __forceinline__ float FcDyn::vjp(const FcGeo& G, const FcLds& L, float t, const float* z, const float* kb, float* yb, float* V, float* pacc, int tid, float*) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, n = G.n, DP = G.DP;
    const size_t FS = (size_t)G.MP * 16;
    // slots: Y_0..Y_n | v_1..v_n | m_1..m_{n-1} (slot n unused) | m_0-bar (= w) .. m_{n-1}-bar | q_1..q_n (d_l-bar .* phi_l'') | a-bar x 2 | lf
    auto Ys = [&](int l) { return V + (size_t)l * FS; };
    auto Vs = [&](int l) { return V + (size_t)(n + l) * FS; };
    auto Ms = [&](int l) { return V + (size_t)(2 * n + l) * FS; };
    auto MBs = [&](int l) { return V + (size_t)(3 * n + 1 + l) * FS; };
    auto Qs = [&](int l) { return V + (size_t)(4 * n + l) * FS; };
    float *AB0 = V + (size_t)(5 * n + 1) * FS, *AB1 = AB0 + FS, *LF = AB1 + FS;
    float *cv = L.red + 80, *l1v = L.red + 96, *l2v = L.red + 112;      // per column: -ll, l1, l2
    for (int idx = tid; idx < DP * 16; idx += kFtThreads) {
        const int r = idx >> 4;
        Ys(0)[idx] = r < D ? z[idx] : 0.f;
        LF[idx] = r < D ? kb[idx] : 0.f;
    }
    if (tid < 16) {
        cv[tid] = -kb[D * 16 + tid];
        l1v[tid] = KIN ? kb[(D + 1) * 16 + tid] : 0.f;
        l2v[tid] = KIN ? kb[(D + 2) * 16 + tid] : 0.f;
    }
    __syncthreads();
    // primal: y_l; the last layer's epilogue forms lf = lz + 2 l1 f (this lane owns the entry)
    for (int l = 1; l <= n; ++l) {
        const float *wt = L.W + G.voff[l - 1], *b = wt + G.outp[l - 1];
        const int out = G.dims[l], code = G.act[l - 1];
        float* y = Ys(l);
        ft_fwd(L.W + G.woff[l - 1], G.ld[l - 1], G.inp[l - 1], G.outp[l - 1], Ys(l - 1), wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = r0 + j, ix = o * 16 + c;
                const float a = o < out ? act_fwd(code, fmaf(wt[o], t, v[j] + b[o])) : 0.f;
                y[ix] = a;
                if constexpr (KIN)
                    if (l == n) LF[ix] = o < D ? fmaf(2.f * l1v[c], a, LF[ix]) : 0.f;
            }
        });
        __syncthreads();
    }
    // the VJP going down: v_n = d_n .* e, m_l = W_{l+1}' v_{l+1}, v_l = d_l .* m_l
    for (int idx = tid; idx < G.outp[n - 1] * 16; idx += kFtThreads) Vs(n)[idx] = act_dy(G.act[n - 1], Ys(n)[idx]) * L.E[idx];
    __syncthreads();
    for (int l = n - 1; l >= 1; --l) {
        const float* y = Ys(l);
        float *m = Ms(l), *vv = Vs(l);
        const int code = G.act[l - 1];
        ft_tr(L.W + G.woff[l], G.ld[l], G.inp[l], G.outp[l], Vs(l + 1), wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; m[ix] = v[j]; vv[ix] = v[j] * act_dy(code, y[ix]); }
        });
        __syncthreads();
    }
    // w = -ll e + 2 l2 eJ (eJ = W_1' v_1)
    {
        float* w = MBs(0);
        if constexpr (KIN) {
            ft_tr(L.W + G.woff[0], G.ld[0], G.inp[0], G.outp[0], Vs(1), wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; w[ix] = fmaf(2.f * l2v[c], v[j], cv[c] * L.E[ix]); }
            });
        } else {
            for (int idx = tid; idx < DP * 16; idx += kFtThreads) w[idx] = cv[idx & 15] * L.E[idx];
        }
        __syncthreads();
    }
    // up the chain: v_l-bar = W_l m_{l-1}-bar; m_l-bar = d_l .* v_l-bar; q_l = d_l-bar .* phi_l'' with d_l-bar = m_l .* v_l-bar (m_n = e)
    for (int l = 1; l <= n; ++l) {
        const float *y = Ys(l), *m = l < n ? Ms(l) : L.E;
        float *mb = l < n ? MBs(l) : nullptr, *q = Qs(l);
        const int code = G.act[l - 1];
        ft_fwd(L.W + G.woff[l - 1], G.ld[l - 1], G.inp[l - 1], G.outp[l - 1], MBs(l - 1), wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ix = (r0 + j) * 16 + c;
                const float yy = y[ix];
                if (mb) mb[ix] = v[j] * act_dy(code, yy);
                q[ix] = m[ix] * v[j] * act_d2y(code, yy);
            }
        });
        __syncthreads();
    }
    // the primal walk: a_n-bar = lf .* d_n + q_n, then layer by layer down to z-bar
    float *ab = AB0, *abn = AB1;
    float tsum = 0.f;
    for (int idx = tid; idx < G.outp[n - 1] * 16; idx += kFtThreads) ab[idx] = fmaf(LF[idx], act_dy(G.act[n - 1], Ys(n)[idx]), Qs(n)[idx]);
    __syncthreads();
    for (int l = n; l >= 1; --l) {
        const int in = G.dims[l - 1], out = G.dims[l];
        float* pl = pacc + G.off[l - 1];
        ft_wgrad(Vs(l), MBs(l - 1), ab, Ys(l - 1), G.outp[l - 1], G.inp[l - 1], out, in, pl, wave, lane);
        for (int o = tid; o < out; o += kFtThreads) {
            float s = 0.f;
            for (int k = 0; k < 16; ++k) s += ab[o * 16 + k];
            if (G.td) { pl[in * out + o] += t * s; tsum = fmaf(L.W[G.voff[l - 1] + o], s, tsum); }
            pl[(in + G.td) * out + o] += s;
        }
        if (l > 1) {
            const float *y = Ys(l - 1), *q = Qs(l - 1);
            const int code = G.act[l - 2];
            ft_tr(L.W + G.woff[l - 1], G.ld[l - 1], G.inp[l - 1], G.outp[l - 1], ab, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; abn[ix] = fmaf(v[j], act_dy(code, y[ix]), q[ix]); }
            });
        } else {
            ft_tr(L.W + G.woff[0], G.ld[0], G.inp[0], G.outp[0], ab, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int r = r0 + j; if (r < D) yb[r * 16 + c] += v[j]; }
            });
        }
        __syncthreads();
        float* s = ab; ab = abn; abn = s;
    }
    return tsum;
}

}  // namespace rnde
