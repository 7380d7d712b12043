// dxrl_pg_rollout.h -- what the fused policy-gradient rollout kernels share (dxrl_pg.hip: the
// 64-env reference kernel k_pg_rollout; dxrl_pg_rollout16.hip: the 16-env kernel k_pg_rollout_ws;
// dxrl_pg_rollout8.hip: the 32-env kernel k_pg_rollout_e8 for >= 32 envs per CU): the launch
// arguments, the episode bookkeeping and tape helpers, the choice of a template instantiation, the
// LDS-only barrier and the hidden-row swizzle.  No reference counterpart beyond the env step
// itself.
#pragma once
#include <type_traits>

#include "dxrl_gemm.h"
#include "dxrl_pg.h"

namespace dxrl {

constexpr float kLog2Pi = 1.8378770664093453f;

struct PgRolloutArgs {
    EnvSoA s;
    Weights w;
    int max_episode_steps, max_steps, horizon;
    const bf16* wbf;
    const float* params;
    uint64_t env_seed, policy_seed;
    int64_t gid0;
    uint64_t iteration;
    float obs_noise, dyn_noise;
    bf16* obs_rm;   // [(T+1) N][kIn]
    bf16* obs_fm;   // [kIn][T N]
    float* act;     // [T N][kActPad]
    float* logp;    // [T N]
    float* rew;     // [T N]
    uint8_t* done;  // [T N]
    double* ep_ret; // [N] open-episode return (persists across calls)
    int32_t* ep_count;
    double* ep_sum_ret;
    int32_t* ep_sum_len;
    int32_t* ep_succ;
    int diag;       // timing ablations: bit0 skip actor MLP, bit1 skip env step
    int success_terminated;
    int record_cap;
    double* rec_return;
    int32_t* rec_length;
    uint8_t* rec_success;
    int32_t* rec_end_step;
    uint16_t* ep_code;   // [T N] scheduler feed: 0, or (episode length << 1) | success (nullable)
    float* applied_act;  // [T N][kActPad] the action the env integrated (nullable; parity checks)
    float* dyn_noise_tape;  // [T N][kActPad] f32(sigma) * z as added to the action (nullable; ws kernel)
    float* obs_noise_tape;  // [(T+1) N][kObsNoiseLd] f32(sigma) * z per observation element (nullable)
    bf16* h2_tape;          // [T N][kH2Ld] the actor's layer-2 activations of every step (nullable)
    unsigned long long* stamps;  // diag & 128: cycles per step segment (16- / 32-env kernels)
};
constexpr int kObsNoiseLd = 48;
constexpr int kH2Ld = 264;  // h2_tape row pitch (bf16): the fused learner's H2 tile rows (kHp)

// Workgroup barrier for LDS hand-offs only: __syncthreads() also drains every outstanding
// global store (s_waitcnt vmcnt(0)) before s_barrier, which puts the tape stores' write
// latency on each step's critical path.  Nothing here is handed between waves through global
// memory, so only LDS is fenced.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// hidden rows of 256 bf16 with their 16-byte chunks XOR-swizzled by the row (chunk c of row r < 16
// at chunk c ^ r; the 32-row kernel swizzles row 16 + r like row r): 16-lane fragment reads
// conflict-free, 8-byte epilogue stores 2-way
__device__ __forceinline__ int swz16(int r, int col) { return ((((col >> 3) ^ r) << 3) | (col & 7)); }

// An env's episode bookkeeping over one launch: the open episode's return (persists across
// launches) and the launch's episode count and sums.  One lane per env keeps it (the env's lane in
// k_pg_rollout, the aux twin's lanes in the lane-split kernels, `lead` the one that writes).
struct EpisodeBook {
    double ep_ret = 0.0, sum_ret = 0.0;
    int32_t cnt = 0, sum_len = 0, succ = 0;

    // step t of env i settled: reward r, episode end `done` with te (terminated, 0 / 1) and the
    // episode's length len -- the reward tape, the first record_cap episode records, the sums
    __device__ __forceinline__ void settle_step(const PgRolloutArgs& p, double r, int32_t done, int32_t te, int32_t len,
                                                int64_t t, int64_t i, bool lead) {
        ep_ret += r;
        if (lead) p.rew[t * p.s.n + i] = (float)r;
        if (done) {
            if (lead && cnt < p.record_cap) {
                const int64_t o = i * p.record_cap + cnt;
                p.rec_return[o] = ep_ret;
                p.rec_length[o] = len;
                p.rec_success[o] = p.success_terminated ? (uint8_t)te : (uint8_t)0;
                p.rec_end_step[o] = (int32_t)t;
            }
            ++cnt;
            sum_ret += ep_ret;
            sum_len += len;
            succ += te;
            ep_ret = 0.0;
        }
    }
    __device__ __forceinline__ void store(const PgRolloutArgs& p, int64_t i) const {
        p.ep_ret[i] = ep_ret;
        p.ep_count[i] = cnt;
        p.ep_sum_ret[i] = sum_ret;
        p.ep_sum_len[i] = sum_len;
        p.ep_succ[i] = succ;
    }
};

// the step-end bytes of sample m: done, and the scheduler feed (episode length << 1) | success
__device__ __forceinline__ void write_step_end(const PgRolloutArgs& p, int64_t m, bool done, bool te, int32_t len) {
    p.done[m] = done;
    if (p.ep_code)
        p.ep_code[m] = done ? (uint16_t)((len << 1) | (p.success_terminated && te ? 1 : 0)) : (uint16_t)0;
}

// parity tape of the observation noise: block blk (elements 4 blk .. 4 blk + 3) of env i's
// observation row `row`, the values the observation row adds (f32(sigma) * z; 0 past kObs)
__device__ __forceinline__ void write_obs_noise_tape(const PgRolloutArgs& p, int64_t row, int64_t i, int blk,
                                                     const float nz[4]) {
    float4 v;
    v.x = 4 * blk + 0 < kObs ? p.obs_noise * nz[0] : 0.0f;
    v.y = 4 * blk + 1 < kObs ? p.obs_noise * nz[1] : 0.0f;
    v.z = 4 * blk + 2 < kObs ? p.obs_noise * nz[2] : 0.0f;
    v.w = 4 * blk + 3 < kObs ? p.obs_noise * nz[3] : 0.0f;
    *reinterpret_cast<float4*>(p.obs_noise_tape + (row * p.s.n + i) * kObsNoiseLd + 4 * blk) = v;
}

// Host: f(kNoise, kDiag, kDense) with the three switches as std::integral_constant<bool, .>, so a
// launcher names its kernel template once.  kNoise: fused noise or the noise parity tapes; kDiag:
// diag_flags / parity tapes set; kDense: the env's reward.
template <class F>
void with_rollout_switches(bool noise, bool diag, bool dense, F&& f) {
    const auto pick = [](bool b, auto&& g) { b ? g(std::true_type{}) : g(std::false_type{}); };
    pick(noise, [&](auto kNoise) {
        pick(diag, [&](auto kDiag) { pick(dense, [&](auto kDense) { f(kNoise, kDiag, kDense); }); });
    });
}

// The 16-env rollout (dxrl_pg_rollout16.hip): one workgroup of 8 waves per 16 envs, each env on the
// 16 lanes of a DPP row.  The 32-env rollout (dxrl_pg_rollout8.hip): 32 envs per workgroup, each
// on 8 lanes.  Same tapes, records and env state bit for bit.
constexpr int kLsEnvs = 16, kE8Envs = 32;
int launch_pg_rollout_ws(const PgRolloutArgs& p, int64_t n, bool noise, bool diag, bool dense, hipStream_t st);
int launch_pg_rollout_e8(const PgRolloutArgs& p, int64_t n, bool noise, bool diag, bool dense, hipStream_t st);

}  // namespace dxrl
