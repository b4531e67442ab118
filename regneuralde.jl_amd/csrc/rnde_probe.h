// rnde_probe.h -- rnde_debug_elementwise (include/rnde.h): the element-wise device functions called one at a time, out[i] = fn(in[i]).
// The functions live in three headers, and rnde_latent.h / rnde_ffjord.h each belong to one translation unit, so the entry point (rnde.hip)
// runs the functions of rnde_device.h itself and asks rnde_latent.hip and rnde_ffjord.hip for theirs.  Every kernel here calls the function
// in its header: there is no second copy of any formula.
#pragma once
#include <hip/hip_runtime.h>

namespace rnde {

// the selectors (rnde_elementwise_fn of include/rnde.h, which static_asserts cannot reach from here: rnde.hip checks them)
enum { EW_TANH_FAST = 0, EW_TANH_FAST2_X = 1, EW_TANH_FAST2_Y = 2, EW_PRE_FWD = 3, EW_PRE_BWD = 4, EW_ACT_FWD = 5, EW_ACT_DY = 6, EW_ACT_D2Y = 7,
       EW_TANH_F = 8, EW_SIGMOID_F = 9, EW_FF_SOFTPLUS = 10 };

// out[i] = f(in[i], in2[i]) (in2 NULL: 0), grid-stride
template <class F>
static __global__ __launch_bounds__(256) void rnde_elementwise_kernel(const F f, const float* __restrict__ in, const float* __restrict__ in2,
                                                                      const long long n, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = f(in[i], in2 ? in2[i] : 0.f);
}
template <class F>
static inline hipError_t elementwise_launch(const F f, const float* in, const float* in2, long long n, float* out, hipStream_t s) {
    const long long want = (n + 255) / 256;
    hipLaunchKernelGGL(rnde_elementwise_kernel<F>, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, s, f, in, in2, n, out);
    return hipGetLastError();
}

hipError_t elementwise_latent(int fn, const float* in, long long n, float* out, hipStream_t s);      // rnde_latent.hip: tanh_f, sigmoid_f
hipError_t elementwise_ffjord(const float* in, long long n, float* out, hipStream_t s);               // rnde_ffjord.hip: ff_softplus

}  // namespace rnde
