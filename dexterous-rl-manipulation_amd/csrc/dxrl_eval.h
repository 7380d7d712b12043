// dxrl_eval.h -- what the evaluation episode-program kernels share (dxrl_eval.hip: k_eval /
// k_eval_ls, the reference's three policies; dxrl_eval_mlp.hip: k_eval_mlp, the frozen MLP actor):
// the launch parameters, the noise stream id and the lane-split geometry.
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

// lane-split programs: a row of 16 lanes per env, 16 rows (4 waves) per workgroup
constexpr int kEvalRows = 16, kEvalThreads = 16 * kEvalRows;

}  // namespace dxrl
