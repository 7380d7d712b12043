// dxrl_keep_best.h -- the conditional parameter copy behind the keep-best rules of the training
// log (dxrl_pg_log.hip) and of both validation rows (dxrl_pg_val_common.h).  A header of its own,
// beside dxrl_reduce.h: a kernel defined in a header is compiled into every translation unit that
// includes it, and the summaries launch none.
#pragma once
#include "dxrl_reduce.h"

namespace dxrl {
namespace {

constexpr int kCopyThreads = 256;

// params -> best iff *flag (a row's is_best column) is set; a thread per quad of floats: a 16-byte
// copy where both pointers allow and the quad is whole, scalar otherwise.  (The name is the
// validation's, whose form this is.)
__global__ __launch_bounds__(kCopyThreads) void k_pg_val_keep_best(const double* __restrict__ flag,
                                                                   const float* __restrict__ params,
                                                                   float* __restrict__ best, int64_t n, int vec) {
    if (*flag == 0.0) return;
    const int64_t i = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x;
    if (vec && 4 * i + 4 <= n) {
        reinterpret_cast<float4*>(best)[i] = reinterpret_cast<const float4*>(params)[i];
    } else {
        for (int64_t k = 4 * i; k < 4 * i + 4 && k < n; ++k) best[k] = params[k];
    }
}

inline int launch_keep_best(hipStream_t st, const double* flag, const float* params, float* best, int64_t n) {
    const int64_t quads = (n + 3) / 4;
    hipLaunchKernelGGL(k_pg_val_keep_best, dim3((unsigned)((quads + kCopyThreads - 1) / kCopyThreads)),
                       dim3(kCopyThreads), 0, st, flag, params, best, n, (int)(aligned16(params) && aligned16(best)));
    return launch_check("k_pg_val_keep_best");
}

}  // namespace
}  // namespace dxrl
