// dxrl_moments.h -- (count, mean, M2) triples: the only home of the moments arithmetic of every
// translation unit that reduces means and variances on the device (dxrl_pg_gae.hip, dxrl_pg_log.hip,
// dxrl_pg_val*.hip and the four dxrl_*_summary.hip).
//
// Moments without cancellation: M2 is the sum of squared deviations about the mean; triples are
// merged with Chan et al.'s pairwise update in a fixed order (deterministic).  A plain
// sum(x^2) - mean sum(x) loses ~(mean/std)^2 ulps (2.8e-6 relative at mean/std = 4.6e4).
//
// push(m, x) and merge(m, Moments{1.0, x, 0.0}) are the same mathematics and not the same bits
// (d / n1 against d * (1 / n)): a caller keeps the form it has.
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
// Welford step: one value into a running triple
__device__ __forceinline__ void push(Moments& m, double x) {
    const double n1 = m.n + 1.0, d = x - m.mean;
    m.mean += d / n1;
    m.m2 += d * (x - m.mean);
    m.n = n1;
}
// fixed-order wave merge by lane shuffles (offsets 32, 16, .., 1); lane 0 holds the result
__device__ __forceinline__ Moments wave_moments(Moments v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const Moments b{__shfl_down(v.n, o, 64), __shfl_down(v.mean, o, 64), __shfl_down(v.m2, o, 64)};
        v = merge(v, b);
    }
    return v;
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
