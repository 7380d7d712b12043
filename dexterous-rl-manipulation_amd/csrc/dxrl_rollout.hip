// dxrl_rollout.hip -- fused multi-step rollout with per-env SimpleLearner.
//
// Replaces the run_episode loop (training/episode_utils.py:13-55) driving a
// SimpleLearner (policies/simple_learner.py:49-99) over consecutive episodes.
// One lane = one env + its learner; T steps run inside one launch with all
// state in registers (loaded once, stored once), so a 200-step rollout costs
// one launch instead of 200 x (select, step, update) round trips.
//
// RNG: parity mode consumes host tapes (legacy MT19937 gauss values for the
// learner, resolved PCG64 reset draws for the env) with the reference's
// data-dependent consumption order; throughput mode draws from per-env
// Philox4x32-10 streams on device.
//
// k_rollout_curriculum is the same loop with a curriculum scheduler per lane
// (evaluation/curriculum_ablation.py:62-73): see "curriculum study" below.
#include "dxrl_internal.h"

using namespace dxrl;

namespace dxrl {

struct LearnerSoA {
    float* mean;
    double* best;
    double* ep_return;
    uint64_t* noise_ctr;
    int64_t n;
};

static int learner_layout(int64_t n, dxrl_learner_layout* L) {
    auto a256 = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
    int64_t off = 0;
    L->mean = off;
    off = a256(off + 4 * kD * n);
    L->best = off;
    off = a256(off + 8 * n);
    L->ep_return = off;
    off = a256(off + 8 * n);
    L->noise_ctr = off;
    off = a256(off + 8 * n);
    L->total_bytes = off;
    return DXRL_OK;
}

static LearnerSoA learner_soa(void* base, int64_t n) {
    dxrl_learner_layout L;
    learner_layout(n, &L);
    char* b = static_cast<char*>(base);
    return LearnerSoA{reinterpret_cast<float*>(b + L.mean), reinterpret_cast<double*>(b + L.best),
                      reinterpret_cast<double*>(b + L.ep_return), reinterpret_cast<uint64_t*>(b + L.noise_ctr), n};
}

__global__ void k_learner_init(LearnerSoA L) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n) return;
#pragma unroll
    for (int k = 0; k < kD; ++k) L.mean[k * L.n + i] = 0.0f;  // SL:46
    L.best[i] = -__builtin_inf();                             // SL:47
    L.ep_return[i] = 0.0;
    L.noise_ctr[i] = 0;
}

__global__ void k_learner_reset(LearnerSoA L, const uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n || (mask && !mask[i])) return;
    L.best[i] = -__builtin_inf();  // SL:97-99
    L.ep_return[i] = 0.0;
}

// SL:59-71 for N learners: a = clip(mean + f32(0 + s*g), -1, 1)
__global__ void k_learner_select(LearnerSoA L, double noise, const double* __restrict__ gauss,
                                 float* __restrict__ act) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n) return;
#pragma unroll
    for (int k = 0; k < kD; ++k)
        act[i * kD + k] = clipf(L.mean[k * L.n + i] + (float)(0.0 + noise * gauss[i * kD + k]), -1.0f, 1.0f);
}

// SL:82-95 for the masked learners: mean = clip(f32(f64(mean) + (0 + lr*g)), +-clip); best = r
__global__ void k_learner_update(LearnerSoA L, double lr, float clip, const double* __restrict__ gauss,
                                 const double* __restrict__ reward, const uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n || !mask[i]) return;
#pragma unroll
    for (int k = 0; k < kD; ++k) {
        const float m = (float)((double)L.mean[k * L.n + i] + (0.0 + lr * gauss[i * kD + k]));
        L.mean[k * L.n + i] = clipf(m, -clip, clip);
    }
    L.best[i] = reward[i];
}

struct RolloutParams {
    Weights w;
    int max_episode_steps;
    int max_steps;  // run_episode loop bound (episode_utils.py:38-42)
    int num_steps;
    int success_terminated;
    double lr, noise, clip;
    uint64_t env_seed, learner_seed;
    int64_t gid0;
};

// Fill g[0..kD) with the next kD normals of this env's learner stream.
template <bool kTape>
__device__ __forceinline__ bool draw_normals(double* g, const double* tape_row, int64_t stride, int& cur,
                                             uint32_t k0, uint32_t k1, uint64_t& ctr) {
    if (kTape) {
        if (cur + kD > stride) return false;
#pragma unroll
        for (int k = 0; k < kD; ++k) g[k] = tape_row[cur + k];
        cur += kD;
    } else {
#pragma unroll
        for (int b = 0; b < (kD + 3) / 4; ++b) {
            const u32x4 r = philox(u32x4{(uint32_t)ctr, (uint32_t)(ctr >> 32), kStreamPolicy, 0u}, k0, k1);
            ++ctr;
            float n0, n1, n2, n3;
            box_muller(r.x, r.y, n0, n1);
            box_muller(r.z, r.w, n2, n3);
            if (4 * b + 0 < kD) g[4 * b + 0] = n0;
            if (4 * b + 1 < kD) g[4 * b + 1] = n1;
            if (4 * b + 2 < kD) g[4 * b + 2] = n2;
            if (4 * b + 3 < kD) g[4 * b + 3] = n3;
        }
    }
    return true;
}

template <bool kDense, bool kTape>
__global__ __launch_bounds__(64) void k_rollout_simple(EnvSoA s, LearnerSoA L, RolloutParams p, dxrl_rollout_io io) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    Env e;
    load_env(s, i, e);
    float mean[kD];
#pragma unroll
    for (int k = 0; k < kD; ++k) mean[k] = L.mean[k * L.n + i];
    double best = L.best[i];
    double ep_ret = L.ep_return[i];
    uint64_t nctr = L.noise_ctr[i];
    uint64_t rctr = s.reset_ctr[i];
    uint32_t ek0, ek1, lk0, lk1;
    env_key(p.env_seed, p.gid0 + i, ek0, ek1);
    env_key(p.learner_seed, p.gid0 + i, lk0, lk1);
    const double* grow = kTape ? io.gauss + i * io.gauss_stride : nullptr;
    const double* rrow = kTape ? io.reset_draws + i * io.reset_stride : nullptr;
    int gcur = 0, done_eps = 0;
    const int budget = io.episode_budget ? io.episode_budget[i] : 0x7fffffff;
    bool ok = true;
    const float fnoise = (float)p.noise, fclip = (float)p.clip;

    for (int step = 0; step < p.num_steps && done_eps < budget; ++step) {
        // select_action (SL:59-71)
        double g[kD];
        if (!draw_normals<kTape>(g, grow, io.gauss_stride, gcur, lk0, lk1, nctr)) {
            ok = false;
            break;
        }
        float a[kD];
#pragma unroll
        for (int k = 0; k < kD; ++k) {
            const float nz = kTape ? (float)(0.0 + p.noise * g[k]) : fnoise * (float)g[k];
            a[k] = clipf(mean[k] + nz, -1.0f, 1.0f);
        }
        bool te, tr;
        double cp[4];
        const double r = env_step(e, a, kDense, p.w, p.max_episode_steps, te, tr, cp);
        ep_ret += r;  // episode_utils.py:45 (f64, sequential)
        // update (SL:82-95)
        if (r > best) {
            if (!draw_normals<kTape>(g, grow, io.gauss_stride, gcur, lk0, lk1, nctr)) {
                ok = false;
                break;
            }
#pragma unroll
            for (int k = 0; k < kD; ++k) {
                const float m = kTape ? (float)((double)mean[k] + (0.0 + p.lr * g[k]))
                                      : mean[k] + (float)p.lr * (float)g[k];
                mean[k] = clipf(m, -fclip, fclip);
            }
            best = r;
        }
        if (te || tr || e.t >= p.max_steps) {  // episode_utils.py:42,51-53
            if (done_eps < io.record_cap) {
                const int64_t o = i * io.record_cap + done_eps;
                if (io.ep_return) io.ep_return[o] = ep_ret;
                if (io.ep_length) io.ep_length[o] = e.t;  // step + 1
                if (io.ep_success) io.ep_success[o] = p.success_terminated ? (uint8_t)te : (uint8_t)0;
                if (io.ep_end_step) io.ep_end_step[o] = step;
            }
            if (done_eps + 1 >= budget) {  // the driver's loop ends here: no further env.reset()
                ++done_eps;
                best = -__builtin_inf();
                ep_ret = 0.0;
                break;
            }
            // next run_episode: env.reset() (no seed) + policy.reset()
            const dxrl_curriculum cu = s.curricula[e.cfg];
            if (kTape) {
                if ((int64_t)(done_eps + 1) * kReset > io.reset_stride) {
                    ok = false;
                    break;
                }
                double d[kReset];
#pragma unroll
                for (int k = 0; k < kReset; ++k) d[k] = rrow[done_eps * kReset + k];
                env_reset(e, d, cu);
            } else {
                env_reset_philox(e, cu, ek0, ek1, rctr);
            }
            ++rctr;
            ++done_eps;
            best = -__builtin_inf();
            ep_ret = 0.0;
        }
    }
    store_env(s, i, e);
    s.reset_ctr[i] = rctr;
#pragma unroll
    for (int k = 0; k < kD; ++k) L.mean[k * L.n + i] = mean[k];
    L.best[i] = best;
    L.ep_return[i] = ep_ret;
    L.noise_ctr[i] = nctr;
    if (io.ep_count) io.ep_count[i] = done_eps;
    if (io.gauss_used) io.gauss_used[i] = gcur;
    if (!ok && io.status) atomicOr(io.status, 1);
}

// ---------------------------------------------------------------- curriculum study
// k_rollout_simple with a per-lane curriculum scheduler applied where the episodes end
// (evaluation/curriculum_ablation.py:62-73: run_episode, scheduler.update, env.curriculum_config =
// scheduler.get_current_config()).  One lane = one training run; a lane's group (study arm) names
// the rule and the rows of the env's curriculum table that hold the arm's levels.  The rule runs
// in integers only: the levels' f64 arithmetic is the host's (it fills the table).
struct StudySoA {
    uint64_t* mask;
    int64_t* steps;
    int32_t* episodes;
    int32_t* level;
    int32_t* milestone;
};

static int study_layout(int64_t n, dxrl_study_layout* L) {
    auto a256 = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
    int64_t off = 0;
    L->window_mask = off;
    off = a256(off + 8 * n);
    L->total_steps = off;
    off = a256(off + 8 * n);
    L->total_episodes = off;
    off = a256(off + 4 * n);
    L->level = off;
    off = a256(off + 4 * n);
    L->milestone = off;
    off = a256(off + 4 * n);
    L->total_bytes = off;
    return DXRL_OK;
}

static StudySoA study_soa(void* base, int64_t n) {
    dxrl_study_layout L;
    study_layout(n, &L);
    char* b = static_cast<char*>(base);
    return StudySoA{reinterpret_cast<uint64_t*>(b + L.window_mask), reinterpret_cast<int64_t*>(b + L.total_steps),
                    reinterpret_cast<int32_t*>(b + L.total_episodes), reinterpret_cast<int32_t*>(b + L.level),
                    reinterpret_cast<int32_t*>(b + L.milestone)};
}

__global__ void k_study_init(StudySoA S, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    S.mask[i] = 0;  // CurriculumScheduler.reset (curriculum_scheduler.py:265-273)
    S.steps[i] = 0;
    S.episodes[i] = 0;
    S.level[i] = 0;
    S.milestone[i] = 0;
}

struct StudyParams {
    StudySoA S;
    const dxrl_study_group* groups;  // device
    int32_t num_groups;
    int32_t n_curricula;             // rows of the env's table (bound of every row switch)
    const int32_t* lane_group;
    const int64_t* lane_stream;      // Philox stream id per lane (nullable: gid0 + lane)
    int32_t* ep_level;
};

template <bool kDense, bool kTape>
__global__ __launch_bounds__(64) void k_rollout_curriculum(EnvSoA s, LearnerSoA L, RolloutParams p, dxrl_rollout_io io,
                                                           StudyParams q) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    Env e;
    load_env(s, i, e);
    float mean[kD];
#pragma unroll
    for (int k = 0; k < kD; ++k) mean[k] = L.mean[k * L.n + i];
    double best = L.best[i];
    double ep_ret = L.ep_return[i];
    uint64_t nctr = L.noise_ctr[i];
    uint64_t rctr = s.reset_ctr[i];
    const int64_t sid = q.lane_stream ? q.lane_stream[i] : p.gid0 + i;
    uint32_t ek0, ek1, lk0, lk1;
    env_key(p.env_seed, sid, ek0, ek1);
    env_key(p.learner_seed, sid, lk0, lk1);
    const double* grow = kTape ? io.gauss + i * io.gauss_stride : nullptr;
    const double* rrow = kTape ? io.reset_draws + i * io.reset_stride : nullptr;
    int gcur = 0, done_eps = 0;
    const int budget = io.episode_budget ? io.episode_budget[i] : 0x7fffffff;
    bool ok = true, bad = false;
    const float fnoise = (float)p.noise, fclip = (float)p.clip;

    // the lane's scheduler (state) and its arm (constants)
    uint64_t sc_mask = q.S.mask[i];
    int64_t sc_steps = q.S.steps[i];
    int32_t sc_eps = q.S.episodes[i], sc_k = q.S.level[i], sc_m = q.S.milestone[i];
    int32_t mode = DXRL_STUDY_FIXED, min_succ = 0, num_levels = 0, first_row = 0, num_ms = 0, window = 0;
    int64_t min_eps = 0;
    uint64_t wmask = 0;
    const int64_t* ms = nullptr;
    {
        const int32_t gi = q.lane_group[i];
        if (gi < 0 || gi >= q.num_groups) {
            bad = true;  // runs as a fixed lane
        } else {
            const dxrl_study_group* G = q.groups + gi;
            mode = G->mode;
            window = G->window;
            min_succ = G->min_successes;
            num_levels = G->num_levels;
            first_row = G->first_row;
            num_ms = G->num_milestones < DXRL_STUDY_MAX_MILESTONES ? G->num_milestones : DXRL_STUDY_MAX_MILESTONES;
            min_eps = G->min_episodes;
            wmask = window >= 64 ? ~0ull : (window > 0 ? (1ull << window) - 1ull : 0ull);
            ms = G->milestones;
        }
    }

    for (int step = 0; step < p.num_steps && done_eps < budget; ++step) {
        // select_action (SL:59-71)
        double g[kD];
        if (!draw_normals<kTape>(g, grow, io.gauss_stride, gcur, lk0, lk1, nctr)) {
            ok = false;
            break;
        }
        float a[kD];
#pragma unroll
        for (int k = 0; k < kD; ++k) {
            const float nz = kTape ? (float)(0.0 + p.noise * g[k]) : fnoise * (float)g[k];
            a[k] = clipf(mean[k] + nz, -1.0f, 1.0f);
        }
        bool te, tr;
        double cp[4];
        const double r = env_step(e, a, kDense, p.w, p.max_episode_steps, te, tr, cp);
        ep_ret += r;  // episode_utils.py:45 (f64, sequential)
        // update (SL:82-95)
        if (r > best) {
            if (!draw_normals<kTape>(g, grow, io.gauss_stride, gcur, lk0, lk1, nctr)) {
                ok = false;
                break;
            }
#pragma unroll
            for (int k = 0; k < kD; ++k) {
                const float m = kTape ? (float)((double)mean[k] + (0.0 + p.lr * g[k]))
                                      : mean[k] + (float)p.lr * (float)g[k];
                mean[k] = clipf(m, -fclip, fclip);
            }
            best = r;
        }
        if (te || tr || e.t >= p.max_steps) {  // episode_utils.py:42,51-53
            const bool succ = p.success_terminated && te;
            // scheduler.update(success, steps) (curriculum_scheduler.py:141-222, :304-335)
            sc_mask = (sc_mask << 1) | (succ ? 1ull : 0ull);
            sc_steps += e.t;
            sc_eps += 1;
            bool prog = false;
            if (mode == DXRL_STUDY_SUCCESS_WINDOW)
                prog = sc_eps >= min_eps && sc_k < num_levels && sc_eps >= window &&
                       __popcll(sc_mask & wmask) >= min_succ;
            else if (mode == DXRL_STUDY_STEP_MILESTONES)
                prog = sc_m < num_ms && sc_steps >= ms[sc_m];
            if (prog) {
                const int32_t row = first_row + sc_k + 1;
                if (row >= 0 && row < q.n_curricula) {
                    sc_k += 1;
                    if (mode == DXRL_STUDY_STEP_MILESTONES) sc_m += 1;
                    e.cfg = row;  // env.curriculum_config = ...: read by the next reset (curriculum_ablation.py:67-68)
                } else {
                    bad = true;
                }
            }
            if (done_eps < io.record_cap) {
                const int64_t o = i * io.record_cap + done_eps;
                if (io.ep_return) io.ep_return[o] = ep_ret;
                if (io.ep_length) io.ep_length[o] = e.t;  // step + 1
                if (io.ep_success) io.ep_success[o] = (uint8_t)succ;
                if (io.ep_end_step) io.ep_end_step[o] = step;
                if (q.ep_level) q.ep_level[o] = sc_k;  // difficulty_levels.append (curriculum_ablation.py:73)
            }
            if (done_eps + 1 >= budget) {  // the driver's loop ends here: no further env.reset()
                ++done_eps;
                best = -__builtin_inf();
                ep_ret = 0.0;
                break;
            }
            // next run_episode: env.reset() (no seed) + policy.reset()
            const dxrl_curriculum cu = s.curricula[e.cfg];
            if (kTape) {
                if ((int64_t)(done_eps + 1) * kReset > io.reset_stride) {
                    ok = false;
                    break;
                }
                double d[kReset];
#pragma unroll
                for (int k = 0; k < kReset; ++k) d[k] = rrow[done_eps * kReset + k];
                env_reset(e, d, cu);
            } else {
                env_reset_philox(e, cu, ek0, ek1, rctr);
            }
            ++rctr;
            ++done_eps;
            best = -__builtin_inf();
            ep_ret = 0.0;
        }
    }
    store_env(s, i, e);
    s.cfg[i] = e.cfg;  // store_env leaves the row alone: no other kernel changes it
    s.reset_ctr[i] = rctr;
#pragma unroll
    for (int k = 0; k < kD; ++k) L.mean[k * L.n + i] = mean[k];
    L.best[i] = best;
    L.ep_return[i] = ep_ret;
    L.noise_ctr[i] = nctr;
    q.S.mask[i] = sc_mask;
    q.S.steps[i] = sc_steps;
    q.S.episodes[i] = sc_eps;
    q.S.level[i] = sc_k;
    q.S.milestone[i] = sc_m;
    if (io.ep_count) io.ep_count[i] = done_eps;
    if (io.gauss_used) io.gauss_used[i] = gcur;
    if (!ok && io.status) atomicOr(io.status, 1);
    if (bad && io.status) atomicOr(io.status, 2);
}

}  // namespace dxrl

extern "C" {

int dxrl_learner_layout_for(int32_t num_envs, int32_t action_dim, dxrl_learner_layout* out) {
    DXRL_REQUIRE(out && num_envs > 0, "null layout / num_envs <= 0");
    if (action_dim != kD) {
        set_error("this build compiles action_dim=%d (got %d)", kD, action_dim);
        return DXRL_E_UNSUPPORTED;
    }
    return learner_layout(num_envs, out);
}

int dxrl_learner_init(int32_t device, int32_t num_envs, void* learner_state, void* stream) {
    DXRL_REQUIRE(learner_state && num_envs > 0, "null learner state / num_envs <= 0");
    DeviceGuard g(device);
    const int64_t n = num_envs;
    hipLaunchKernelGGL(k_learner_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       learner_soa(learner_state, n));
    return launch_check("k_learner_init");
}

int dxrl_learner_reset(int32_t device, int32_t num_envs, void* learner_state, const uint8_t* mask, void* stream) {
    DXRL_REQUIRE(learner_state && num_envs > 0, "null learner state / num_envs <= 0");
    DeviceGuard g(device);
    const int64_t n = num_envs;
    hipLaunchKernelGGL(k_learner_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       learner_soa(learner_state, n), mask);
    return launch_check("k_learner_reset");
}

int dxrl_learner_select(int32_t device, int32_t num_envs, const void* learner_state, double exploration_noise,
                        const double* gauss, float* actions, void* stream) {
    DXRL_REQUIRE(learner_state && gauss && actions && num_envs > 0, "null argument / num_envs <= 0");
    DeviceGuard g(device);
    const int64_t n = num_envs;
    hipLaunchKernelGGL(k_learner_select, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       learner_soa(const_cast<void*>(learner_state), n), exploration_noise, gauss, actions);
    return launch_check("k_learner_select");
}

int dxrl_learner_update(int32_t device, int32_t num_envs, void* learner_state, double learning_rate,
                        double action_clip_range, const double* gauss, const double* reward, const uint8_t* mask,
                        void* stream) {
    DXRL_REQUIRE(learner_state && gauss && reward && mask && num_envs > 0, "null argument / num_envs <= 0");
    DeviceGuard g(device);
    const int64_t n = num_envs;
    hipLaunchKernelGGL(k_learner_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       learner_soa(learner_state, n), learning_rate, (float)action_clip_range, gauss, reward, mask);
    return launch_check("k_learner_update");
}

int dxrl_rollout_simple(dxrl_env* env, void* learner_state, const dxrl_learner_config* lc, int32_t num_steps,
                        int32_t max_steps, int32_t success_rule, const dxrl_rollout_io* io_in, void* stream) {
    DXRL_REQUIRE(env && learner_state && lc, "null env/learner/config");
    DXRL_REQUIRE(num_steps >= 0, "num_steps must be >= 0");
    DXRL_REQUIRE(max_steps > 0, "max_steps must be > 0");
    dxrl_rollout_io io{};
    if (io_in) io = *io_in;
    const bool tape = io.gauss != nullptr;
    DXRL_REQUIRE(tape == (io.reset_draws != nullptr), "parity mode needs both the gauss and the reset-draw tapes");
    DXRL_REQUIRE(!tape || (io.gauss_stride > 0 && io.reset_stride >= kReset), "bad tape strides");
    DXRL_REQUIRE(io.record_cap >= 0, "record_cap must be >= 0");
    const int64_t n = env->cfg.num_envs;
    RolloutParams p{weights_of(env->cfg),
                    env->cfg.max_episode_steps,
                    max_steps,
                    num_steps,
                    success_rule == DXRL_SUCCESS_TERMINATED,
                    lc->learning_rate,
                    lc->exploration_noise,
                    lc->action_clip_range,
                    env->cfg.seed,
                    lc->seed,
                    env->cfg.global_env_offset};
    DeviceGuard g(env->device);
    const LearnerSoA L = learner_soa(learner_state, n);
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    hipStream_t st = as_stream(stream);
    const bool dense = env->cfg.reward_type == DXRL_REWARD_DENSE;
    if (dense && tape)
        hipLaunchKernelGGL((k_rollout_simple<true, true>), grid, block, 0, st, env->soa, L, p, io);
    else if (dense)
        hipLaunchKernelGGL((k_rollout_simple<true, false>), grid, block, 0, st, env->soa, L, p, io);
    else if (tape)
        hipLaunchKernelGGL((k_rollout_simple<false, true>), grid, block, 0, st, env->soa, L, p, io);
    else
        hipLaunchKernelGGL((k_rollout_simple<false, false>), grid, block, 0, st, env->soa, L, p, io);
    return launch_check("k_rollout_simple");
}

int dxrl_study_layout_for(int32_t num_envs, dxrl_study_layout* out) {
    DXRL_REQUIRE(out && num_envs > 0, "null layout / num_envs <= 0");
    return study_layout(num_envs, out);
}

int dxrl_study_init(int32_t device, int32_t num_envs, void* sched_state, void* stream) {
    DXRL_REQUIRE(sched_state && num_envs > 0, "null scheduler state / num_envs <= 0");
    DeviceGuard g(device);
    const int64_t n = num_envs;
    hipLaunchKernelGGL(k_study_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       study_soa(sched_state, n), n);
    return launch_check("k_study_init");
}

int dxrl_study_set_groups(const dxrl_env* env, const dxrl_study_group* groups, int32_t num_groups, void* groups_dev,
                          void* stream) {
    DXRL_REQUIRE(env && groups && groups_dev, "null env/groups");
    DXRL_REQUIRE(num_groups >= 1 && num_groups <= DXRL_STUDY_MAX_GROUPS, "num_groups %d outside [1, %d]", num_groups,
                 DXRL_STUDY_MAX_GROUPS);
    for (int32_t k = 0; k < num_groups; ++k) {
        const dxrl_study_group& G = groups[k];
        DXRL_REQUIRE(G.mode >= DXRL_STUDY_FIXED && G.mode <= DXRL_STUDY_STEP_MILESTONES, "group %d: unknown mode %d", k,
                     G.mode);
        if (G.mode == DXRL_STUDY_FIXED) continue;
        DXRL_REQUIRE(G.num_levels >= 0 && G.first_row >= 0 && G.first_row + (int64_t)G.num_levels < env->n_curricula,
                     "group %d: rows %d..%lld outside the env's %d-row curriculum table", k, G.first_row,
                     (long long)G.first_row + G.num_levels, env->n_curricula);
        if (G.mode == DXRL_STUDY_SUCCESS_WINDOW) {
            DXRL_REQUIRE(G.window >= 1 && G.window <= 64, "group %d: window %d outside [1, 64]", k, G.window);
            DXRL_REQUIRE(G.min_successes >= 0 && G.min_successes <= G.window + 1, "group %d: min_successes %d outside [0, window + 1]",
                         k, G.min_successes);
        } else {
            DXRL_REQUIRE(G.num_milestones >= 0 && G.num_milestones <= DXRL_STUDY_MAX_MILESTONES,
                         "group %d: %d milestones (at most %d)", k, G.num_milestones, DXRL_STUDY_MAX_MILESTONES);
            DXRL_REQUIRE(G.num_milestones == G.num_levels, "group %d: one level per milestone", k);
            for (int32_t m = 1; m < G.num_milestones; ++m)
                DXRL_REQUIRE(G.milestones[m - 1] <= G.milestones[m], "group %d: milestones must be sorted", k);
        }
    }
    DeviceGuard g(env->device);
    hipStream_t st = as_stream(stream);
    if (int rc = hip_check(hipMemcpyAsync(groups_dev, groups, sizeof(dxrl_study_group) * num_groups,
                                          hipMemcpyHostToDevice, st),
                           "study groups upload"))
        return rc;
    return hip_check(hipStreamSynchronize(st), "study groups sync");
}

int dxrl_rollout_curriculum(dxrl_env* env, void* learner_state, const dxrl_learner_config* lc, int32_t num_steps,
                            int32_t max_steps, int32_t success_rule, const dxrl_rollout_io* io_in,
                            const dxrl_study_args* study, void* stream) {
    DXRL_REQUIRE(env && learner_state && lc && study, "null env/learner/config/study");
    DXRL_REQUIRE(num_steps >= 0, "num_steps must be >= 0");
    DXRL_REQUIRE(max_steps > 0, "max_steps must be > 0");
    DXRL_REQUIRE(study->groups && study->lane_group && study->sched_state, "null groups/lane_group/sched_state");
    DXRL_REQUIRE(study->num_groups >= 1 && study->num_groups <= DXRL_STUDY_MAX_GROUPS, "num_groups %d outside [1, %d]",
                 study->num_groups, DXRL_STUDY_MAX_GROUPS);
    dxrl_rollout_io io{};
    if (io_in) io = *io_in;
    const bool tape = io.gauss != nullptr;
    DXRL_REQUIRE(tape == (io.reset_draws != nullptr), "parity mode needs both the gauss and the reset-draw tapes");
    DXRL_REQUIRE(!tape || (io.gauss_stride > 0 && io.reset_stride >= kReset), "bad tape strides");
    DXRL_REQUIRE(io.record_cap >= 0, "record_cap must be >= 0");
    const int64_t n = env->cfg.num_envs;
    RolloutParams p{weights_of(env->cfg),
                    env->cfg.max_episode_steps,
                    max_steps,
                    num_steps,
                    success_rule == DXRL_SUCCESS_TERMINATED,
                    lc->learning_rate,
                    lc->exploration_noise,
                    lc->action_clip_range,
                    env->cfg.seed,
                    lc->seed,
                    env->cfg.global_env_offset};
    StudyParams q{study_soa(study->sched_state, n), study->groups, study->num_groups, env->n_curricula,
                  study->lane_group, study->lane_stream, study->ep_level};
    DeviceGuard g(env->device);
    const LearnerSoA L = learner_soa(learner_state, n);
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    hipStream_t st = as_stream(stream);
    const bool dense = env->cfg.reward_type == DXRL_REWARD_DENSE;
    if (dense && tape)
        hipLaunchKernelGGL((k_rollout_curriculum<true, true>), grid, block, 0, st, env->soa, L, p, io, q);
    else if (dense)
        hipLaunchKernelGGL((k_rollout_curriculum<true, false>), grid, block, 0, st, env->soa, L, p, io, q);
    else if (tape)
        hipLaunchKernelGGL((k_rollout_curriculum<false, true>), grid, block, 0, st, env->soa, L, p, io, q);
    else
        hipLaunchKernelGGL((k_rollout_curriculum<false, false>), grid, block, 0, st, env->soa, L, p, io, q);
    return launch_check("k_rollout_curriculum");
}

}  // extern "C"
