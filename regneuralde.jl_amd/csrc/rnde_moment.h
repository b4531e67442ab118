// rnde_moment.h -- the moment-matching loss of reference experiments/sde_toy_problem.jl:27-40 and its reverse (include/rnde.h: rnde_moment_loss).
// u is D x T x B column-major (B trajectories of the saved states, diffeqsol_to_3dtrackedarray's layout); for every (d, t) pair
//   mu = sum_b u / B,  var = sum_b (u - mu)^2 / (B - 1)          (Julia's mean(...; dims = 3) and var(...; dims = 3, mean = means))
//   l2_means = mean over pairs of (m - mu)^2,  l2_vars = mean over pairs of (v - var)^2
// and the cotangent of l2_means + l2_vars:
//   u-bar = -2 (m - mu) / (n B) - 4 (v - var) (u - mu) / (n (B - 1))       (n = D T; the term through mu in var vanishes: sum_b (u - mu) = 0)
// ONE workgroup: thread i owns pairs i, i + kMomThreads, ... (consecutive threads read consecutive addresses at each b), sums over b in index order
// in double, and the per-thread loss partials meet in a fixed tree -- the same bits on every run.  The toy's arrays are 2 x 30 x 100.
#pragma once
#include "rnde_device.h"

namespace rnde {

constexpr int kMomThreads = 512;

static __global__ __launch_bounds__(kMomThreads) void rnde_moment_loss_kernel(const float* __restrict__ u, const float* __restrict__ dmean,
                                                                               const float* __restrict__ dvar, int n, int B, float* __restrict__ loss_out,
                                                                               float* __restrict__ ubar) {
    __shared__ double red[2][kMomThreads];
    const int tid = threadIdx.x;
    double lm = 0.0, lv = 0.0;
    const double inv_n = 1.0 / (double)n, inv_b = 1.0 / (double)B, inv_b1 = 1.0 / (double)(B - 1);
    for (int i = tid; i < n; i += kMomThreads) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += (double)u[(size_t)b * n + i];
        const double mu = s * inv_b;
        double q = 0.0;
        for (int b = 0; b < B; ++b) { const double e = (double)u[(size_t)b * n + i] - mu; q += e * e; }
        const double var = q * inv_b1;
        const double em = (double)dmean[i] - mu, ev = (double)dvar[i] - var;
        lm += em * em; lv += ev * ev;
        if (ubar) {
            const double cm = -2.0 * em * inv_n * inv_b, cv = -4.0 * ev * inv_n * inv_b1;
            for (int b = 0; b < B; ++b) {
                const size_t e = (size_t)b * n + i;
                ubar[e] = (float)(cm + cv * ((double)u[e] - mu));
            }
        }
    }
    red[0][tid] = lm; red[1][tid] = lv;
    __syncthreads();
    for (int w = kMomThreads / 2; w > 0; w >>= 1) {
        if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { loss_out[0] = (float)(red[0][0] * inv_n); loss_out[1] = (float)(red[1][0] * inv_n); }
}

// Flux.Optimise.AdaBelief (include/rnde.h: rnde_adabelief_step; experiments/sde_toy_problem.jl:65): no bias correction, the new m inside (g - m)
static __global__ __launch_bounds__(256) void rnde_adabelief_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                     float* __restrict__ sv, long long len, float gscale, float eta, float b1, float b2,
                                                                     float eps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const float gs = g[i] * gscale;
    const float mn = b1 * m[i] + (1.f - b1) * gs;
    const float d = gs - mn;
    const float sn = b2 * sv[i] + (1.f - b2) * d * d;
    m[i] = mn; sv[i] = sn;
    p[i] = p[i] - eta * mn / (sqrtf(sn) + eps);
}

}  // namespace rnde
