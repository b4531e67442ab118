// rnde_head_eval.h -- the evaluation head of ClassifierNODE in ONE launch: postode Dense(D, C) on the end state of an untaped solve and, with
// labels, the argmax match counted into a device integer (include/rnde.h: rnde_node_classifier_predict).
// Replaces, for evaluation: reference src/models/supervised_classification.jl:44-45 (postode) and src/metrics.jl:2-9 (argmax on both sides,
// `==`, sum) as experiments/mnist_node.jl:185-186, :250-251 call them over both loaders at the end of every epoch.
//
// The logits are rnde_head_col_kernel's (rnde_head.h), operation for operation: one workgroup of four waves per column, thread tid owns the
// rows d = tid + 256 k (k < 4), one fmaf chain over k per class starting from 0, wave_sum_f (the fixed DPP tree of rnde_device.h) within
// each wave, then ((r0 + r1) + (r2 + r3)) + b over the four waves' sums.  So evaluation and training give the same bits from the same u.
// The count (COUNT): thread 0 holds all C logits behind the combine; it takes the FIRST index of the largest logit and the first index of the
// largest entry of the column of y (strict >, Julia's argmax) and adds 1 to *correct with one integer atomic when they are equal.  No float
// atomics.  The counter ACCUMULATES, so the host queues the counting variant exactly once per call, behind the solve's final status (a solve
// that is redone would count twice otherwise); the variant without labels only overwrites its output and is queued in front of the host's wait.
#pragma once
#include "rnde_head.h"

namespace rnde {

// CC > 0: the number of classes as a compile-time constant (10 for the reference's classifier), CC = 0: any C <= kHeadMaxC
template <int CC, bool COUNT>
__global__ __launch_bounds__(256) void rnde_head_eval_kernel(const float* __restrict__ u, const float* __restrict__ p3, const float* __restrict__ y,
                                                             int D, int C, float* __restrict__ logits_out, unsigned long long* __restrict__ correct) {
    constexpr int NC = CC ? CC : kHeadMaxC;
    if (CC) C = CC;
    __shared__ float red[4][kHeadMaxC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = blockIdx.x;
    const float* W = p3;
    const float* b = p3 + (size_t)C * D;
    const float* uc = u + (size_t)c * D;
    float wv[kHeadRowsPerThread][NC], uv[kHeadRowsPerThread];
#pragma unroll
    for (int k = 0; k < kHeadRowsPerThread; ++k) {
        const int d = tid + 256 * k;
        uv[k] = d < D ? uc[d] : 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) wv[k][i] = (i < C && d < D) ? W[(size_t)d * C + i] : 0.f;
    }
    float acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        acc[i] = 0.f;
#pragma unroll
        for (int k = 0; k < kHeadRowsPerThread; ++k) acc[i] = fmaf(wv[k][i], uv[k], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) if (i < C) { const float s = wave_sum_f(acc[i]); if (lane == 0) red[w][i] = s; }
    __syncthreads();
    if (tid != 0) return;
    float* zo = logits_out + (size_t)c * C;
    const float* yc = COUNT ? y + (size_t)c * C : nullptr;
    int iz = 0, iy = 0;
    float mz = 0.f, my = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) if (i < C) {
        const float z = ((red[0][i] + red[1][i]) + (red[2][i] + red[3][i])) + b[i];
        zo[i] = z;
        if (COUNT) {
            const float yv = yc[i];
            if (i == 0) { mz = z; my = yv; }
            if (z > mz) { mz = z; iz = i; }
            if (yv > my) { my = yv; iy = i; }
        }
    }
    if (COUNT && iz == iy) atomicAdd(correct, 1ull);
}

}  // namespace rnde
