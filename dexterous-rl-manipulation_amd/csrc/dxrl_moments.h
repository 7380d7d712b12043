// dxrl_moments.h -- (count, mean, M2) triples and their merge, shared by the translation units
// that reduce means and variances on the device (dxrl_pg.hip: advantage normalisation;
// dxrl_pg_log.hip: the per-iteration training log).
//
// Moments without cancellation: M2 is the sum of squared deviations about the mean; triples are
// merged with Chan et al.'s pairwise update in a fixed order (deterministic).  A plain
// sum(x^2) - mean sum(x) loses ~(mean/std)^2 ulps (2.8e-6 relative at mean/std = 4.6e4).
#pragma once
#include <hip/hip_runtime.h>

namespace dxrl {

struct Moments {
    double n, mean, m2;
};
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
    const double n = a.n + b.n;
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double d = b.mean - a.mean;
    return Moments{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}
// workgroup tree merge in LDS (fixed pairing), result in red[0]
template <int NT>
__device__ void block_merge(Moments v, Moments* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = merge(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
}

}  // namespace dxrl
