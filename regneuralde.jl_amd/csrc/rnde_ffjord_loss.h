// rnde_ffjord_loss.h -- the loss terms and the seeds of the reverse sweep of rnde_ffjord_nll_grad (include/rnde.h), between the taped
// forward solve and its reverse sweep.  The loss is the reference's loss_function (experiments/ffjord_tabular.jl:143-147,
// ffjord_gaussian.jl:142-146):
//
//     loss = -mean(logpx) + lambda_r * mean(sv.saveval) + lambda_k * mean(lambda1) + lambda_j * mean(lambda2)
//
// The loss-and-seed kernel, rnde_ffjord_loss_seed_kernel<KIN>: one workgroup of 256 threads, queued directly behind the solve launch, in
// front of the forward's host wait.  Thread i adds elements i, i + 256, ... in double, in rising index; the 256 partials are combined in
// a fixed tree; the result depends on the values and on B only.  It writes
//     terms_dev[0] = (float)(-sum(logpx) / B)
//     terms_dev[1..2] = (float)(sum(lambda1) / B), (float)(sum(lambda2) / B), which are 0 outside mode 2
//     logpx_bar[b] = -1.0f / (float)B
//     in mode 2, reg_bar[0][b] = lambda_k / (float)B and reg_bar[1][b] = lambda_j / (float)B
// The two seed arrays are fp32, with one fp32 division each; they go into buffers the handle owns.  A NaN in logpx stays a NaN in the
// term.  Plain vector stores, no atomics, no meeting.  When the solve fails, its output is simply not used.
//
// On the host, after the step log has been read (n = the number of saved values, including the 0 at init when cb_save_start is set):
//     *reg_out_host = (float)((double)lambda_r * sum(saveval) / n), summed in double in log order; 0 on regularize = 0 handles
//     saveval_bar[i] = lambda_r / (float)n, one fp32 division
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace rnde {

constexpr int kFfLossThreads = 256;

// What the forward hands to the kernel behind its solve launch.  reg / reg_bar: 2 x B, row stride B (KIN only).
struct FfLossSeed {
    const float* logpx;
    const float* reg;
    float* terms;           // 3 floats
    float* logpx_bar;       // B
    float* reg_bar;         // 2 x B
    int B;
    float lambda_k, lambda_j;
};

template <bool KIN>
static __global__ __launch_bounds__(kFfLossThreads) void rnde_ffjord_loss_seed_kernel(FfLossSeed Q) {
    constexpr int NS = KIN ? 3 : 1;
    __shared__ double part[NS][kFfLossThreads];
    const int tid = threadIdx.x, B = Q.B;
    double acc[NS];
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    for (int b = tid; b < B; b += kFfLossThreads) {
        acc[0] += (double)Q.logpx[b];
        if constexpr (KIN) {
            acc[1] += (double)Q.reg[b];
            acc[2] += (double)Q.reg[(size_t)B + b];
        }
    }
    for (int k = 0; k < NS; ++k) part[k][tid] = acc[k];
    __syncthreads();
    for (int s = kFfLossThreads / 2; s > 0; s >>= 1) {      // the fixed tree: partial i takes partial i + s
        if (tid < s)
            for (int k = 0; k < NS; ++k) part[k][tid] += part[k][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        Q.terms[0] = (float)(-part[0][0] / (double)B);
        if constexpr (KIN) {
            Q.terms[1] = (float)(part[1][0] / (double)B);
            Q.terms[2] = (float)(part[2][0] / (double)B);
        } else {
            Q.terms[1] = 0.f;
            Q.terms[2] = 0.f;
        }
    }
    const float fb = (float)B;
    const float lb = __fdiv_rn(-1.0f, fb);
    for (int b = tid; b < B; b += kFfLossThreads) Q.logpx_bar[b] = lb;
    if constexpr (KIN) {
        const float kb = __fdiv_rn(Q.lambda_k, fb), jb = __fdiv_rn(Q.lambda_j, fb);
        for (int b = tid; b < B; b += kFfLossThreads) { Q.reg_bar[b] = kb; Q.reg_bar[(size_t)B + b] = jb; }
    }
}

static inline void ff_launch_loss_seed(const FfLossSeed& Q, bool kin, hipStream_t s) {
    if (kin) hipLaunchKernelGGL(rnde_ffjord_loss_seed_kernel<true>, dim3(1), dim3(kFfLossThreads), 0, s, Q);
    else hipLaunchKernelGGL(rnde_ffjord_loss_seed_kernel<false>, dim3(1), dim3(kFfLossThreads), 0, s, Q);
}

// The host half: the saved values' loss term and their cotangents, by the formulas above.  sv: n saved values in log order.
static inline float ff_saveval_term(const float* sv, int n, float lambda_r, std::vector<float>& sv_bar) {
    sv_bar.assign((size_t)(n > 0 ? n : 0), 0.f);
    if (n < 1) return 0.f;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += (double)sv[i];
    const float bar = lambda_r / (float)n;
    for (int i = 0; i < n; ++i) sv_bar[i] = bar;
    return (float)((double)lambda_r * sum / (double)n);
}

}  // namespace rnde
