// rnde_bnode_tile.h -- the reverse sweep of rnde_node_tile_solve_kernel: discretise-then-optimise through every Tsit5 stage of every accepted
// step, one workgroup per tile, every accepted step in one launch, no meeting.  Step sizes and times are constants of the sweep
// (track_ctrl = track_initdt = 0, as on every TrackedFFJORD engine): once the step log is fixed no column depends on another, and the
// cotangent of a saved value EEst * dt reaches the stages through EEst, whose value comes from the step log.  Differentiating the controller
// on this layout would take one meeting per reversed step; rnde_node_create_tiled refuses the two track flags by name.
//
// The stages are recomputed from the taped uprev with the forward's own evaluation (NtDyn::eval).  One stage's VJP, cotangent kb of
// f(y, t), notation of rnde_ffjordc.h (d_l = phi_l' taken from the layer's output):
//     v_n = d_n .* kb,   v_l = d_l .* W_{l+1}' v_{l+1},   yb += W_1' v_1
//     W_l-bar += v_l y_{l-1}',   wt_l-bar += t sum_c v_l,   b_l-bar += sum_c v_l        (outer products over the tile's 16 columns)
// The transposed products are ft_tr, the outer products one v_mfma_f32_16x16x4_f32 chain per 16 x 16 block of W_l (k = the 16 columns).
// Parameter cotangents accumulate in the tile's own row of pacc ([ntiles][P]) by plain read-modify-write: every entry has one owner lane
// for the whole sweep, no atomics; rnde_node_tile_reduce_kernel then sums the tiles in tile order in double (the arithmetic of
// rnde_ffjordt_reduce_kernel, restated here: that header defines kernels only one translation unit may hold).
#pragma once
#include "rnde_node_tile.h"

namespace rnde {

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
// calls it; ends behind a barrier.
__device__ __forceinline__ void nt_vjp(const FcGeo& G, const NtLds& L, float t, const float* y, const float* kb, float* yb, float* pacc, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, n = G.n;
    for (int idx = tid; idx < D * 16; idx += kFtThreads) L.X[idx] = y[idx];      // (rows >= D of L.X are zero and stay so)
    __syncthreads();
    fc_chain(G, L.W, L.X, L.Y, t, wave, lane, [](int, int, float) {});
    float *va = L.V0, *vb = L.V1;
    {
        const float* yn = L.Y + G.yoff[n - 1];
        const int code = G.act[n - 1];
        for (int idx = tid; idx < G.outp[n - 1] * 16; idx += kFtThreads) va[idx] = (idx >> 4) < D ? act_dy(code, yn[idx]) * kb[idx] : 0.f;
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
            if (G.td) pl[in * out + o] += t * s;
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
}

__global__ __launch_bounds__(kFtThreads) void rnde_node_tile_reverse_kernel(const NodeTileRevParams Q) {
    extern __shared__ float nt_smem[];
    const FcGeo& G = Q.G;
    const int tile = blockIdx.x, tid = threadIdx.x, D = G.D, Bp = Q.Bp, col0 = tile * 16, nel = D * 16;
    const NtLds L = NtDyn::lds(G, nt_smem);
    FcDyn::load_params(G, Q.p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) L.X[idx] = 0.f;
    float* ws = Q.ws + (size_t)tile * NtDyn::rev_ws_floats(G);
    const size_t RS = (size_t)nel;
    auto Ys = [&](int s) { return ws + (size_t)s * RS; };
    auto Ks = [&](int s) { return ws + (size_t)(7 + s) * RS; };
    auto Kb = [&](int s) { return ws + (size_t)(14 + s) * RS; };
    float *UB = ws + 21 * RS, *UBn = ws + 22 * RS, *Yb = ws + 23 * RS;
    float* pacc = Q.pacc + (size_t)tile * G.P;
    for (int q = tid; q < G.P; q += kFtThreads) pacc[q] = 0.f;
    const size_t RB = (size_t)D * Bp;
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        UB[idx] = col < Q.B ? Q.u_bar[(size_t)col * D + r] : 0.f;
    }
    __syncthreads();      // pacc and L.X are next touched by other threads (the entries' owner lanes, the stage loop)
    const double N = (double)D * (double)Q.B;
    for (int n = Q.n_acc - 1; n >= 0; --n) {
        const NtStepRec st = Q.rec[n];
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
                L.X[idx] = y;
            }
            NtDyn::eval(G, L, t + kTsC[s] * dt, Ks(s), 16, tid);
        }
        for (int idx = tid; idx < nel; idx += kFtThreads) {
            for (int s = 0; s < 7; ++s) Kb(s)[idx] = 0.f;
            UBn[idx] = 0.f;
            Yb[idx] = UB[idx];                                // cotangent of unew = stage-7 input
        }
        // ---- A: reverse of the error estimate (the saved value EEst * dt; rnde_ffjord_tile.h) ----
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
            nt_vjp(G, L, t + kTsC[s] * dt, Ys(s), Kb(s), Yb, pacc, tid);
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
            if (col < Q.B) Q.x_bar[(size_t)col * D + r] = UB[idx];
        }
}

// p_bar[q] = sum over tiles of pacc[tile][q], in tile order, carried in double
static __global__ __launch_bounds__(256) void rnde_node_tile_reduce_kernel(const float* __restrict__ pacc, int P, int ntiles, float* __restrict__ p_bar) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P) return;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s += (double)pacc[(size_t)t * P + q];
    p_bar[q] = (float)s;
}

}  // namespace rnde
