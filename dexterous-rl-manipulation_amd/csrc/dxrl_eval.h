// dxrl_eval.h -- what the evaluation episode-program kernels share (dxrl_eval.hip: k_eval /
// k_eval_ls, the reference's three policies; dxrl_eval_mlp.hip: k_eval_mlp, the frozen MLP actor):
// the launch parameters, the noise stream id, the history moments and the lane-split geometry.
// The lane-split episode program itself (k_eval_ls, k_eval_mlp) and the host side of the two
// entry points are in dxrl_eval_row.h.
#pragma once
#include "dxrl_internal.h"

namespace dxrl {

constexpr uint32_t kStreamEvalNoise = 0x45564e00u;

struct EvalParams {
    Weights w;
    int max_episode_steps;  // env truncation (ME:245)
    int dense;
    int has_object;         // env constructed with object_position (ME:28, :156-161)
    int n_curricula;
    double obj[3];
    dxrl_eval_args a;
    unsigned long long* diag_iters;  // DXRL_EVAL_DIAG: step iterations executed per wave, summed
};

// History moments of an episode's per-step contact counts c (0..5), kept in two dwords beside the
// step loop so that no history row has to reach HBM (dxrl_eval_args.hist_moments):
//   lo  bits 0-14 S1 = sum c (<= 20,480), bits 15-31 S2 = sum c^2 (<= 102,400)
//   hi  bits 0-14 the last five counts, 3 bits each (newest lowest), bits 15-19 F = the
//       first-five sum, bits 20-22 the peak
// which holds for max_steps <= 4096 (kHistMomentsMaxSteps; the entry points check it).
constexpr int kHistMomentsMaxSteps = 4096;
struct HistAcc {
    uint32_t lo, hi;
};
__device__ __forceinline__ void hist_acc_step(HistAcc& h, uint32_t c, int step) {
    h.lo += c + ((c * c) << 15);
    const uint32_t f = ((h.hi >> 15) & 31u) + (step < 5 ? c : 0u);
    const uint32_t pk = max((h.hi >> 20) & 7u, c);
    h.hi = (((h.hi << 3) | c) & 0x7fffu) | (f << 15) | (pk << 20);
}
// i32 [5]: S1, S2, F, L (the sum of the last five counts), peak
__device__ __forceinline__ void hist_acc_store(const HistAcc& h, int32_t* __restrict__ out) {
    uint32_t l = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) l += (h.hi >> (3 * k)) & 7u;
    out[0] = (int32_t)(h.lo & 0x7fffu);
    out[1] = (int32_t)(h.lo >> 15);
    out[2] = (int32_t)((h.hi >> 15) & 31u);
    out[3] = (int32_t)l;
    out[4] = (int32_t)((h.hi >> 20) & 7u);
}

// lane-split programs: a row of 16 lanes per env, 16 rows (4 waves) per workgroup
constexpr int kEvalRows = 16, kEvalThreads = 16 * kEvalRows;

}  // namespace dxrl
