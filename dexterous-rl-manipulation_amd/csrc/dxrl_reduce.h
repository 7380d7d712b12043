// dxrl_reduce.h -- the wave and workgroup helpers of the device summaries (the four
// dxrl_*_summary.hip, dxrl_pg_log.hip, dxrl_pg_val*.hip): fixed-order lane reductions, the quiet
// NaN, the alignment test and the ordered compaction of flagged rows into a list.  The moments
// arithmetic is in dxrl_moments.h, the conditional parameter copy in dxrl_keep_best.h.
#pragma once
#include "dxrl_internal.h"

namespace dxrl {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// fixed-order wave reductions by lane shuffles (offsets 32, 16, .., 1); lane 0 holds the result
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int b = __shfl_down(v, o, 64);
        v = b < v ? b : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int b = __shfl_down(v, o, 64);
        v = b > v ? b : v;
    }
    return v;
}
// the same over doubles that are not NaN (a lane without a value passes +inf / -inf)
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double b = __shfl_down(v, o, 64);
        v = b < v ? b : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double b = __shfl_down(v, o, 64);
        v = b > v ? b : v;
    }
    return v;
}

// The flagged rows of [0, rows) listed in ascending order by one workgroup of NT threads: thread t
// owns rows [t c, (t + 1) c), counts its flagged rows (first(r), called once per row), an inclusive
// Hillis-Steele scan in `scan` (NT ints of LDS) gives its place, and a second walk (again(r))
// writes them.  tie_count gets the true count, also when the list overflowed (status bit 1).
// kSkipEmpty: a thread that counted nothing does not walk again (for a predicate that costs).
template <int NT, bool kSkipEmpty, class First, class Again>
__device__ __forceinline__ void compact_rows(int rows, First first, Again again, int* scan,
                                             int32_t* __restrict__ tie_count, int32_t* __restrict__ tie_list,
                                             int tie_cap, int32_t* __restrict__ status) {
    const int tid = threadIdx.x;
    const int c = (rows + NT - 1) / NT;
    const int lo = min(tid * c, rows), hi = min(lo + c, rows);
    int cnt = 0;
    for (int r = lo; r < hi; ++r) cnt += first(r);
    scan[tid] = cnt;
    __syncthreads();
    for (int s = 1; s < NT; s <<= 1) {
        const int v = tid >= s ? scan[tid - s] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int at = scan[tid] - cnt;
    if (!kSkipEmpty || cnt)
        for (int r = lo; r < hi; ++r)
            if (again(r)) {
                if (at < tie_cap) tie_list[at] = r;
                ++at;
            }
    if (tid == NT - 1) {
        *tie_count = scan[tid];
        if (scan[tid] > tie_cap) atomicOr(status, 2);
    }
}
// a cheap predicate asked twice
template <int NT, class Pred>
__device__ __forceinline__ void compact_rows(int rows, Pred pred, int* scan, int32_t* __restrict__ tie_count,
                                             int32_t* __restrict__ tie_list, int tie_cap,
                                             int32_t* __restrict__ status) {
    compact_rows<NT, false>(rows, pred, pred, scan, tie_count, tie_list, tie_cap, status);
}

}  // namespace dxrl
