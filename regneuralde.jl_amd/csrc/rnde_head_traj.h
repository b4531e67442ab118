// rnde_head_traj.h -- ClassifierNSDE with several sample paths per input, on the device: the repeat of the batch, postsde Dense(D, C) with
// the trajectory mean, logitcrossentropy and their reverse, the fold of the repeated input's cotangent, and the count of correct predictions.
// Replaces, for the classifier: reference src/models/supervised_classification.jl:92 and :102-103 (repeat), :96-98 (postsde, mean over the
// trajectories), experiments/mnist_nsde.jl's Flux.Losses.logitcrossentropy, the Tracker reverse of all of them, and src/metrics.jl:2 (argmax
// against the labels).  The solve between the repeat and the head is rnde_sde.h / rnde_sdemw.h, untouched.
//
// Layout: column j = t B + b of the expanded batch is trajectory t of input b (what Julia's repeat(x, 1, T) gives), T trajectories, B inputs.
//   p3 = Flux.destructure(Dense(D, C)) = [vec(W) (C x D, column-major); b (C)]   (as rnde_head.h)
//   z_tb = W u_tb + b3;  z_b = (1/T) sum_t z_tb;  ce = (1/B) sum_b -sum_i y_ib logsoftmax(z_b)_i
//   delta_b = (softmax(z_b) sum_i y_ib - y_b) / B        (y need not be one-hot)
//   u-bar_tb = W^T delta_b / T;  W-bar = (1/T) sum_{t,b} delta_b u_tb^T;  b-bar = sum_b delta_b
//
// The averaged logits are accumulated in fp64 and rounded to fp32 once; the softmax takes its differences z_i - max z from the fp64 values, so
// the size of the logits costs the probabilities no bits.  Everything behind that is fp32.
//
// The order of every sum (no float atomics anywhere; the same bits run to run):
//   z_tb[i]   lane l of a wave owns rows d = l, l + 64, ..: one fp64 fma chain over them in increasing d from 0 (the products of two floats are
//             exact there), then wave_sum_d over the 64 lanes (rnde_device.h: the fixed DPP tree), then + b3[i].
//   z_b[i]    wave w of the input's workgroup owns trajectories t = w, w + 4, .. and adds their z_tb[i] in increasing t from 0; the four
//             waves' sums combine as (w0 + w1) + (w2 + w3); one division by T; all in fp64, then rounded to fp32.
//   sum_i     over the classes (max, sum of exp, sum of y, cross entropy): i = 0 .. C - 1 in that order, in every thread alike.
//   u-bar     one fmaf chain over i = 0 .. C - 1 from 0, one division by T; the same value is stored to all T columns of the input.
//   W-bar     s_b[d] = sum_t u_tb[d], t = 0 .. T - 1 in that order from u_0b[d]; then sum_b delta_b[i] s_b[d] exactly as rnde_head.h sums
//             sum_c delta_c[i] u_c[d]: rnde_head_wgrad_kernel (kHeadChunks chunks of consecutive inputs, one fmaf chain in increasing b
//             each), the chunks' partials added in increasing chunk order from 0; one division by T.
//   b-bar[i]  lane l adds delta_b[i] over b = l, l + 64, .. in increasing b, then wave_sum_f.  ce: the same over the per-input values, / B.
//   fold      x-bar_b[d] = sum_t x-bar_{tB+b}[d], t = 0 .. T - 1 in that order from the t = 0 value.
#pragma once
#include "rnde_head.h"

namespace rnde {

// D x B -> D x (B T): column j is a copy of column j mod B, i.e. element e of the output is element e mod (D B) of the input
static __global__ __launch_bounds__(256) void rnde_traj_expand_kernel(const float* __restrict__ x, float* __restrict__ xe, long long DB, long long n) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) xe[e] = x[e % DB];
}

// x-bar_b = sum_t x-bar_{tB+b}: element e < D B of the output is the sum of elements e + t D B of the input, t = 0 .. T - 1 in that order
static __global__ __launch_bounds__(256) void rnde_traj_fold_kernel(const float* __restrict__ xe_bar, float* __restrict__ x_bar, long long DB, int T) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < DB; e += (long long)gridDim.x * 256) {
        float s = xe_bar[e];
        for (int t = 1; t < T; ++t) s += xe_bar[e + (long long)t * DB];
        x_bar[e] = s;
    }
}

// one workgroup (4 waves) per input b.  GRAD = false: the averaged logits only (rnde_nsde_classifier_predict; y, ubar, delta, ce_col, usum unused)
template <bool GRAD>
__global__ __launch_bounds__(256) void rnde_head_traj_col_kernel(const float* __restrict__ u, const float* __restrict__ p3, const float* __restrict__ y,
                                                                 int D, int C, int B, int T, float* __restrict__ logits_out,
                                                                 float* __restrict__ ubar, float* __restrict__ delta, float* __restrict__ ce_col,
                                                                 float* __restrict__ usum) {
    __shared__ double red[4][kHeadMaxC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    const float* W = p3;
    const float* b3 = p3 + (size_t)C * D;
    double zs[kHeadMaxC];
#pragma unroll
    for (int i = 0; i < kHeadMaxC; ++i) zs[i] = 0.0;
    for (int t = w; t < T; t += 4) {
        const float* uc = u + ((size_t)t * B + b) * D;
        double acc[kHeadMaxC];
#pragma unroll
        for (int i = 0; i < kHeadMaxC; ++i) acc[i] = 0.0;
        for (int d = lane; d < D; d += 64) {
            const double uv = (double)uc[d];
#pragma unroll
            for (int i = 0; i < kHeadMaxC; ++i) if (i < C) acc[i] = fma((double)W[(size_t)d * C + i], uv, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < kHeadMaxC; ++i) if (i < C) zs[i] += wave_sum_d(acc[i]) + (double)b3[i];
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kHeadMaxC; ++i) if (i < C) red[w][i] = zs[i];
    }
    __syncthreads();
    const float fT = (float)T;
    double zd[kHeadMaxC], mxd = -1.0e300;
#pragma unroll
    for (int i = 0; i < kHeadMaxC; ++i) {
        zd[i] = i < C ? ((red[0][i] + red[1][i]) + (red[2][i] + red[3][i])) / (double)T : 0.0;
        if (i < C) mxd = fmax(mxd, zd[i]);
    }
    if (tid == 0 && logits_out)
        for (int i = 0; i < C; ++i) logits_out[(size_t)b * C + i] = (float)zd[i];
    if (!GRAD) return;
    float e[kHeadMaxC], se = 0.f, sy = 0.f;      // e_i = z_i - max z <= 0
#pragma unroll
    for (int i = 0; i < kHeadMaxC; ++i) {
        e[i] = (float)(zd[i] - mxd);
        if (i < C) { se += expf(e[i]); sy += y[(size_t)b * C + i]; }
    }
    const float lse = logf(se);
    float ce = 0.f, dl[kHeadMaxC];
    const float fB = (float)B;
#pragma unroll
    for (int i = 0; i < kHeadMaxC; ++i) {
        dl[i] = 0.f;
        if (i < C) {
            const float yv = y[(size_t)b * C + i];
            const float lp = e[i] - lse;      // logsoftmax(z_b)_i
            ce -= yv * lp;
            dl[i] = (expf(lp) * sy - yv) / fB;
        }
    }
    if (tid == 0) {
        ce_col[b] = ce;
        for (int i = 0; i < C; ++i) delta[(size_t)b * C + i] = dl[i];
    }
    for (int d = tid; d < D; d += 256) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kHeadMaxC; ++i) if (i < C) s = fmaf(W[(size_t)d * C + i], dl[i], s);
        s /= fT;
        float us = u[(size_t)b * D + d];
        ubar[(size_t)b * D + d] = s;
        for (int t = 1; t < T; ++t) {
            const size_t o = ((size_t)t * B + b) * D + d;
            us += u[o];
            ubar[o] = s;
        }
        usum[(size_t)b * D + d] = us;
    }
}

// pass 2 of W-bar behind rnde_head_wgrad_kernel on (usum, delta): as rnde_head_reduce_kernel, the weight part divided by T
static __global__ __launch_bounds__(256) void rnde_head_traj_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ delta,
                                                                           const float* __restrict__ ce_col, int D, int C, int B, int T,
                                                                           float* __restrict__ p3bar, float* __restrict__ ce_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < C * D) {
        float v[kHeadChunks];
#pragma unroll
        for (int ch = 0; ch < kHeadChunks; ++ch) v[ch] = partial[(size_t)ch * C * D + i];
        float s = 0.f;
#pragma unroll
        for (int ch = 0; ch < kHeadChunks; ++ch) s += v[ch];
        p3bar[i] = s / (float)T;
    }
    if (blockIdx.x == gridDim.x - 1) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        for (int k = w; k < C; k += 4) {
            float s = 0.f;
            for (int c = lane; c < B; c += 64) s += delta[(size_t)c * C + k];
            s = wave_sum_f(s);
            if (lane == 0) p3bar[(size_t)C * D + k] = s;
        }
        if (w == 3) {
            float s = 0.f;
            for (int c = lane; c < B; c += 64) s += ce_col[c];
            s = wave_sum_f(s);
            if (lane == 0) *ce_out = s / (float)B;
        }
    }
}

// Julia's argmax on both sides (src/metrics.jl:2): the FIRST index of the largest averaged logit against the first index of the largest label
// entry; the matches of a wave are counted by ballot and ADDED to *correct with one integer atomic per wave
static __global__ __launch_bounds__(256) void rnde_head_count_kernel(const float* __restrict__ z, const float* __restrict__ y, int C, int B,
                                                                     unsigned long long* __restrict__ correct) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (b < B) {
        int iz = 0, iy = 0;
        float mz = z[(size_t)b * C], my = y[(size_t)b * C];
        for (int i = 1; i < C; ++i) {
            const float zv = z[(size_t)b * C + i], yv = y[(size_t)b * C + i];
            if (zv > mz) { mz = zv; iz = i; }
            if (yv > my) { my = yv; iy = i; }
        }
        hit = iz == iy;
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(correct, (unsigned long long)__popcll(m));
}

}  // namespace rnde
