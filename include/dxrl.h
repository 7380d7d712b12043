/*
 * dxrl.h -- C ABI of the MI355X-native vectorised manipulation-env hot path.
 *
 * Plain C: no torch / HIP types in the signatures.  Device buffers are
 * passed as plain pointers (HBM addresses valid on the env's device); streams
 * as `void*` (a hipStream_t, NULL = the device's null stream).  Every entry
 * point returns DXRL_OK (0) or a negative status; dxrl_last_error() returns a
 * thread-local message for the last failing call.  Calls on one handle are
 * not thread-safe; kernels are stream-ordered and asynchronous.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the I2S9/dexterous-rl-manipulation checkout).
 */
#ifndef DXRL_H_
#define DXRL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXRL_ABI_VERSION 1

/* status codes */
#define DXRL_OK 0
#define DXRL_E_INVALID (-1)     /* bad argument (shape, null pointer, range)  -> ValueError   */
#define DXRL_E_HIP (-2)         /* HIP runtime / launch failure               -> RuntimeError */
#define DXRL_E_UNSUPPORTED (-3) /* configuration this build does not compile   -> ValueError   */
#define DXRL_E_TAPE (-4)        /* a parity tape ran out (see dxrl_rollout_*)  -> RuntimeError */

/* reward plugin selection: envs/manipulation_env.py:64-73 */
#define DXRL_REWARD_SPARSE 0 /* rewards/reward_shaping.py:190-242 SparseReward  */
#define DXRL_REWARD_DENSE 1  /* rewards/reward_shaping.py:12-187  RewardShaping */

/* number of f64 slots of one reset draw record: joints + (size, mass, friction) + spawn xyz */
#define DXRL_RESET_EXTRA 6
#define DXRL_MAX_CURRICULA 256

/* episode success rule of a rollout:
 *   TRAINING   -- training/episode_utils.py:52   info.get("success", False) -> always 0
 *   TERMINATED -- evaluation/evaluator.py:157, robustness_tests.py:303   success = terminated */
#define DXRL_SUCCESS_TRAINING 0
#define DXRL_SUCCESS_TERMINATED 1

/* One curriculum configuration -- experiments/config.py:17-42 (CurriculumConfig).
 * A range is used iff its has_* flag is set (config.py:44-84: one draw each,
 * in the order size, mass, friction).  friction_is_f64_scalar reproduces the
 * NumPy-2 promotion when the friction is a numpy.float64 (scheduler
 * interpolation, experiments/curriculum_scheduler.py:90-139): the velocity
 * damping multiply then runs in f64 (manipulation_env.py:215-216). */
typedef struct dxrl_curriculum {
    double object_size, object_mass, friction_coefficient;
    double size_range[2], mass_range[2], friction_range[2];
    double spawn_x_range[2], spawn_y_range[2], spawn_z_range[2];
    int32_t has_size_range, has_mass_range, has_friction_range, friction_is_f64_scalar;
} dxrl_curriculum;

/* Constructor arguments -- envs/manipulation_env.py:24-34 (+ reward_shaping.py:14-25 weights). */
typedef struct dxrl_env_config {
    int32_t num_envs;          /* N envs on this device (shard)                 */
    int32_t num_fingers;       /* manipulation_env.py:26 (this build: 5)         */
    int32_t joints_per_finger; /* manipulation_env.py:27 (this build: 3)         */
    int32_t max_episode_steps; /* manipulation_env.py:29                         */
    int32_t reward_type;       /* DXRL_REWARD_*  (manipulation_env.py:31)        */
    int32_t has_object_position; /* manipulation_env.py:28 object_position given */
    double object_position[3];
    double distance_weight, contact_weight, closure_weight, stability_weight;
    uint64_t seed;             /* device RNG: env i keyed by (seed, global_env_offset + i) */
    int64_t global_env_offset; /* first global env id of this shard (multi-GPU)  */
} dxrl_env_config;

/* Byte offsets (from the state base) of the struct-of-arrays env state in HBM. */
typedef struct dxrl_env_layout {
    int64_t total_bytes;
    int64_t jp, jv;      /* f32 [D][N]  joint positions / velocities            */
    int64_t op;          /* f64 [3][N]  object position                         */
    int64_t ov;          /* f32 [3][N]  object velocity                         */
    int64_t flags;       /* u32 [N]     contacts | prev<<8 | has_prev<<16 | op_is_f32<<17 | has_object<<18 */
    int64_t step_count;  /* i32 [N]                                              */
    int64_t size, mass, friction; /* f64 [N] current episode curriculum values  */
    int64_t cfg_index;   /* i32 [N]     curriculum table row per env             */
    int64_t reset_ctr;   /* u64 [N]     resets so far (device-RNG counter)       */
    int64_t curricula;   /* dxrl_curriculum [DXRL_MAX_CURRICULA]                 */
} dxrl_env_layout;

typedef struct dxrl_env dxrl_env;

int dxrl_abi_version(void);
const char* dxrl_last_error(void);

/* Layout of the state slab the caller allocates (device memory, 256-B aligned). */
int dxrl_env_layout_for(const dxrl_env_config* cfg, dxrl_env_layout* out);

/* Replaces DexterousManipulationEnv.__init__ (envs/manipulation_env.py:24-122).
 * `state` = caller-owned device slab of layout.total_bytes on `device`.
 * Initialises the SoA (zeros, has_object from cfg) on `stream`. */
int dxrl_env_create(const dxrl_env_config* cfg, int32_t device, void* state, void* stream, dxrl_env** out);
int dxrl_env_destroy(dxrl_env* env);

/* Curriculum table + per-env row (host arrays, copied on `stream`; returns after the copies
 * completed, so the arrays may be temporaries).
 * env_index == NULL -> every env uses row 0.  Takes effect at the next reset,
 * as assigning env.curriculum_config does (evaluation/component_ablation.py:166). */
int dxrl_env_set_curricula(dxrl_env* env, const dxrl_curriculum* table, int32_t n,
                           const int32_t* env_index, void* stream);
/* The same without waiting: the copies are only enqueued on `stream`, so `table` and
 * `env_index` (pinned host memory) must stay unchanged until the stream has passed them
 * (the trainer's scheduler pushes a progression mid-iteration without a host sync). */
int dxrl_env_set_curricula_async(dxrl_env* env, const dxrl_curriculum* table, int32_t n,
                                 const int32_t* env_index, void* stream);

/* Replaces reset(seed, options) (envs/manipulation_env.py:124-182).
 * mask   : device u8 [N] or NULL (all envs)
 * draws  : device f64 [N][D+6] resolved reset draws (parity mode: the host
 *          replays each env's gymnasium PCG64 stream), or NULL -> device Philox.
 *          Slots: D joint uniforms, size, mass, friction, spawn x, y, z (a slot
 *          is read only when the reference would draw it).
 * obs    : device f32 [N][obs_dim] or NULL. */
int dxrl_env_reset(dxrl_env* env, const uint8_t* mask, const double* draws, float* obs, void* stream);

/* Replaces step(action) (envs/manipulation_env.py:184-252) incl. _update_contacts
 * (:285-310), the reward plugin (rewards/reward_shaping.py:50-242),
 * _check_termination (:332-336) and _get_observation (:254-264).
 * actions f32 [N][D]; obs f32 [N][obs_dim] (nullable); reward f64 [N];
 * terminated/truncated u8 [N]; components f64 [N][4] (nullable). */
int dxrl_env_step(dxrl_env* env, const float* actions, float* obs, double* reward,
                  uint8_t* terminated, uint8_t* truncated, double* components, void* stream);

/* The reward plugins' own entry point, for callers outside env.step():
 *   rewards/reward_shaping.py:50-99   RewardShaping.compute(joint_positions, finger_tips,
 *                                     object_position, contacts, num_fingers, joints_per_finger)
 *   rewards/reward_shaping.py:205-242 SparseReward.compute(...)
 * as called at envs/manipulation_env.py:318-325, for `count` independent items.  The dense
 * terms are the step kernels' own dense_reward (csrc/dxrl_device.h) on the given inputs.
 *   weights          HOST f64 [4] distance, contact, closure, stability (dense only);
 *                    every other array is device memory
 *   joint_positions  f32 [count][15]      (the env's f32 joint array, ME:143-145)
 *   finger_tips      f64 [count][5][3]    (ME:296-303)
 *   object_position  f64 [count][3]
 *   contacts         f32 [count][5]       (ME:310; > 0.5 counts as a contact)
 *   prev_contacts    f32 [count][5], has_prev u8 [count]: RewardShaping.prev_contacts (None ==
 *                    has_prev 0), read and updated in place as RS:172-185 does (dense only)
 *   out              f64 [count][5]: total, distance, contact, closure, stability
 * num_fingers / joints_per_finger must be this build's 5 / 3 (DXRL_E_UNSUPPORTED otherwise). */
int dxrl_reward_compute(int32_t device, int32_t reward_type, const double* weights, int64_t count,
                        int32_t num_fingers, int32_t joints_per_finger, const float* joint_positions,
                        const double* finger_tips, const double* object_position, const float* contacts,
                        float* prev_contacts, uint8_t* has_prev, double* out, void* stream);

/* Recompute the observation of the current state (envs/manipulation_env.py:254-264). */
int dxrl_env_observe(dxrl_env* env, float* obs, void* stream);

/* Assigning env.max_episode_steps (read by training/episode_utils.py:38 and
 * the truncation test manipulation_env.py:245). */
int dxrl_env_set_max_episode_steps(dxrl_env* env, int32_t max_episode_steps);

/* SimpleLearner.select_action / update for a batch of independent learners
 * (policies/simple_learner.py:49-95), for callers that drive env.step()
 * themselves (the Gymnasium facade).  gauss = f64 [N][D] standard normals
 * (np.random.normal(0, s) == 0 + s * gauss); update applies to envs whose
 * mask byte is set -- the host decides `reward > best_reward` because it owns
 * the RNG stream whose consumption depends on it. */
int dxrl_learner_select(int32_t device, int32_t num_envs, const void* learner_state, double exploration_noise,
                        const double* gauss, float* actions, void* stream);
int dxrl_learner_update(int32_t device, int32_t num_envs, void* learner_state, double learning_rate,
                        double action_clip_range, const double* gauss, const double* reward, const uint8_t* mask,
                        void* stream);

/* ------------------------------------------------------------------------
 * Fused rollout with per-env SimpleLearner hill-climbers
 * (training/episode_utils.py:13-55 run_episode loop + policies/simple_learner.py:49-99).
 * One launch runs `num_steps` env steps of every env, auto-resetting at
 * episode end (terminated || truncated || step_count == max_steps) exactly as
 * consecutive run_episode() calls do.  State stays in registers across steps.
 * ------------------------------------------------------------------------ */
typedef struct dxrl_learner_layout {
    int64_t total_bytes;
    int64_t mean;        /* f32 [D][N] mean_action                             */
    int64_t best;        /* f64 [N]    best_reward                             */
    int64_t ep_return;   /* f64 [N]    running total_reward of the open episode */
    int64_t noise_ctr;   /* u64 [N]    device-RNG counter                      */
} dxrl_learner_layout;

typedef struct dxrl_learner_config {
    double learning_rate;     /* simple_learner.py:27 */
    double exploration_noise; /* :28 */
    double action_clip_range; /* :29 */
    uint64_t seed;            /* device RNG (Philox) key; the reference uses the global np.random */
} dxrl_learner_config;

typedef struct dxrl_rollout_io {
    /* parity tapes (all NULL -> device Philox streams) */
    const double* gauss;      /* f64 [N][gauss_stride] legacy-MT19937 gauss values per env  */
    int64_t gauss_stride;
    const double* reset_draws;/* f64 [N][reset_stride] consecutive reset records (D+6 each) */
    int64_t reset_stride;
    /* episode records (nullable), [N][record_cap] */
    int32_t record_cap;
    double* ep_return;
    int32_t* ep_length;
    uint8_t* ep_success;
    int32_t* ep_end_step;     /* rollout step index at which the episode ended */
    /* per-env outputs (nullable) */
    int32_t* ep_count;        /* i32 [N] episodes finished in this call   */
    int32_t* gauss_used;      /* i32 [N] tape values consumed             */
    int32_t* status;          /* i32 [1] device error word (tape overrun) */
    /* i32 [N] episode budget of this call (nullable = unbounded): an env stops once it has
       finished that many episodes, before the next episode's env.reset() -- a driver's
       `for episode in range(num_episodes)` loop (evaluation/component_ablation.py:154-166). */
    const int32_t* episode_budget;
} dxrl_rollout_io;

int dxrl_learner_layout_for(int32_t num_envs, int32_t action_dim, dxrl_learner_layout* out);
/* zero mean_action, best_reward = -inf, ep_return = 0 (SimpleLearner.__init__, simple_learner.py:45-47) */
int dxrl_learner_init(int32_t device, int32_t num_envs, void* learner_state, void* stream);
/* policy.reset() for every env: best_reward = -inf (simple_learner.py:97-99) and the
 * open-episode return = 0 (run_episode starts a new episode, episode_utils.py:33-39). */
int dxrl_learner_reset(int32_t device, int32_t num_envs, void* learner_state, const uint8_t* mask, void* stream);
/* learner_state must have been laid out for env's num_envs. */
int dxrl_rollout_simple(dxrl_env* env, void* learner_state, const dxrl_learner_config* lcfg,
                        int32_t num_steps, int32_t max_steps, int32_t success_rule,
                        const dxrl_rollout_io* io, void* stream);

/* ------------------------------------------------------------------------
 * Curriculum-ablation study (evaluation/curriculum_ablation.py:25-134): dxrl_rollout_simple
 * with one CurriculumScheduler per lane, applied on the device where the lane's episodes end,
 * so a run whose difficulty changes between two of its own episodes -- and a whole study of
 * thousands of such runs, both arms -- is one launch.
 *
 * A lane belongs to a GROUP (an arm of the study).  The group names the progression rule and
 * the rows first_row .. first_row + num_levels of the env's curriculum table that hold the
 * arm's levels: the host builds them by stepping a real scheduler (_progress /
 * _interpolate_config, experiments/curriculum_scheduler.py:90-139,188-222), so no f64 level
 * arithmetic runs on the device.  At every episode end the lane runs scheduler.update(success,
 * steps) (curriculum_scheduler.py:141-161) in integers; on a progression its env's row becomes
 * first_row + level, read by the next reset exactly as `env.curriculum_config =
 * scheduler.get_current_config()` (curriculum_ablation.py:67-68) is.
 * ------------------------------------------------------------------------ */
#define DXRL_STUDY_MAX_GROUPS 16
#define DXRL_STUDY_MAX_MILESTONES 64
#define DXRL_STUDY_FIXED 0           /* no scheduler: train_without_curriculum (curriculum_ablation.py:86-134) */
#define DXRL_STUDY_SUCCESS_WINDOW 1  /* CurriculumScheduler._should_progress (curriculum_scheduler.py:163-186)  */
#define DXRL_STUDY_STEP_MILESTONES 2 /* StepBasedScheduler._should_progress  (curriculum_scheduler.py:304-310)  */

/* One arm's scheduler constants (the CurriculumScheduler constructor arguments,
 * curriculum_scheduler.py:22-57, :284-302, reduced to integers by the host). */
typedef struct dxrl_study_group {
    int32_t mode;           /* DXRL_STUDY_*                                                      */
    int32_t window;         /* window_size, 1..64 (SUCCESS_WINDOW)                               */
    int32_t min_successes;  /* smallest count c with c / window >= success_rate_threshold in f64
                               (np.mean of the window's bools, :182-186); 0 when the threshold is
                               <= 0, window + 1 when no count reaches it                          */
    int32_t num_levels;     /* progressions that raise the level (:195-222): the lane stops at
                               level num_levels, where current_difficulty_level >= 1.0 (:175)     */
    int32_t first_row;      /* curriculum-table row of level 0; level k is row first_row + k      */
    int32_t num_milestones; /* STEP_MILESTONES: == num_levels, <= DXRL_STUDY_MAX_MILESTONES       */
    int64_t min_episodes;   /* min_episodes_before_progression (:171)                             */
    int64_t milestones[DXRL_STUDY_MAX_MILESTONES]; /* sorted step_milestones (:301)               */
} dxrl_study_group;

/* Byte offsets of the per-lane scheduler state (device slab, 256-B aligned); persists across
 * calls like the env and learner slabs.  The fields of CurriculumScheduler.reset (:265-273). */
typedef struct dxrl_study_layout {
    int64_t total_bytes;
    int64_t window_mask;    /* u64 [N] episode_successes, newest episode in bit 0                 */
    int64_t total_steps;    /* i64 [N]                                                           */
    int64_t total_episodes; /* i32 [N]                                                           */
    int64_t level;          /* i32 [N] level index k (current_difficulty_level = the host's table[k]) */
    int64_t milestone;      /* i32 [N] current_milestone_idx (:302)                               */
} dxrl_study_layout;

typedef struct dxrl_study_args {
    const dxrl_study_group* groups; /* DEVICE [num_groups], written by dxrl_study_set_groups      */
    int32_t num_groups;
    const int32_t* lane_group;      /* device i32 [N] group of each lane                          */
    void* sched_state;              /* device slab of dxrl_study_layout_for(N)                     */
    int32_t* ep_level;              /* device i32 [N][record_cap] (nullable): the level index after
                                       that episode's update -- difficulty_levels.append(
                                       scheduler.get_difficulty_level()) (curriculum_ablation.py:73) */
    const int64_t* lane_stream;     /* device i64 [N] (nullable = global_env_offset + lane): the id
                                       that keys the lane's Philox streams, so a run's streams do
                                       not depend on the lane it occupies                          */
} dxrl_study_args;

int dxrl_study_layout_for(int32_t num_envs, dxrl_study_layout* out);
/* CurriculumScheduler.reset() for every lane (curriculum_scheduler.py:265-273). */
int dxrl_study_init(int32_t device, int32_t num_envs, void* sched_state, void* stream);
/* Checks the groups (host array) against the env's curriculum table and copies them to
 * groups_dev (device, num_groups entries); returns after the copy completed. */
int dxrl_study_set_groups(const dxrl_env* env, const dxrl_study_group* groups, int32_t num_groups,
                          void* groups_dev, void* stream);
/* dxrl_rollout_simple (same tapes / Philox streams, rewards, success rules, episode_budget,
 * record_cap, gauss_used, resumable state) with the lanes' schedulers.  A DXRL_STUDY_FIXED lane
 * computes what dxrl_rollout_simple computes, bit for bit.  Status word: bit 0 a tape ran out,
 * bit 1 a lane's group or row lies outside its table (the lane then does not progress). */
int dxrl_rollout_curriculum(dxrl_env* env, void* learner_state, const dxrl_learner_config* lcfg,
                            int32_t num_steps, int32_t max_steps, int32_t success_rule,
                            const dxrl_rollout_io* io, const dxrl_study_args* study, void* stream);

/* ------------------------------------------------------------------------
 * bf16 MFMA GEMM used by the actor-critic learner (no reference counterpart;
 * exported for tests and diagnostics).  C[M][N] = epi(A[M][K] . Bt[N][K]^T):
 * bias (bias[n*bias_stride]), act (0 identity / 1 tanh), gate (multiply by
 * 1 - gate[m][n]^2), outputs f32 row-major Cf, bf16 row-major Crm, bf16
 * feature-major Cfm[n][m] (each nullable).  splits > 1: split-K over K into
 * `partial` (f32 [splits + 16][M][N]: the last 16 slabs are the two-level reduction's
 * scratch) reduced into Cf (ld = N).  K % 32 == 0.
 * ------------------------------------------------------------------------ */
int dxrl_gemm_bf16(int32_t device, const void* A, int64_t lda, const void* Bt, int64_t ldb, int64_t M, int32_t N,
                   int32_t K, const float* bias, int64_t bias_stride, int32_t act, const void* gate, int64_t ldg,
                   float* Cf, int64_t ldcf, void* Crm, int64_t ldc, void* Cfm, int64_t ldfm, float* Cffm,
                   int64_t ldffm, int32_t splits, float* partial, void* stream);
/* Weight gradient out[O][I] = sum_m Y[m][o] X[m][i] from row-major bf16 operands
 * (k-major MFMA operands via ds_read_b64_tr_b16); split-K over m into `partial`
 * (f32 [splits + 16][O][I]; the last 16 slabs are reduction scratch) reduced in fixed order
 * (deterministic).  O, I, ldy, ldx % 8 == 0. */
int dxrl_wgrad_bf16(int32_t device, const void* Y, int64_t ldy, int32_t O, const void* X, int64_t ldx, int32_t I,
                    int64_t M, int32_t splits, float* partial, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Policy-gradient learner (NEW capability: the reference has no network,
 * no GAE and no gradient -- SURVEY.md §8(a) A11-A13; parity unpinned vs the
 * reference, pinned by tests against a torch fp32 restatement).
 * Actor 45->256->256->15 (tanh) + state-independent log_std; critic
 * 45->256->256->1.  Master parameters f32 (dxrl_pg_sizes().params elements,
 * padded blocks, see csrc/dxrl_pg.h), bf16 packed copies for the MFMA GEMMs.
 * ------------------------------------------------------------------------ */
int dxrl_pg_sizes(int64_t* params, int64_t* packed_bf16);
int dxrl_pg_pack_weights(int32_t device, const float* params, void* packed, void* stream);

typedef struct dxrl_pg_rollout_args {
    int32_t horizon;           /* env steps per env in this call (T)                       */
    int32_t max_steps;         /* run_episode loop bound (episode_utils.py:38-42)          */
    uint64_t policy_seed;      /* Philox key of the action / noise streams                 */
    uint64_t iteration;        /* Philox counter base (iteration * T + t)                  */
    double obs_noise_std;      /* robustness_tests.py:199-207 (0 = off)                    */
    double dyn_noise_std;      /* robustness_tests.py:180-187 (0 = off)                    */
    void* obs_rm;              /* bf16 [(T+1) N][64] policy inputs (+ bootstrap row block) */
    void* obs_fm;              /* bf16 [64][T N] feature-major copy (nullable)             */
    float* act;                /* f32 [T N][16] sampled (pre-clip) actions                 */
    float* logp;               /* f32 [T N] log pi(a|s) at sampling time                   */
    float* rew;                /* f32 [T N]                                                */
    uint8_t* done;             /* u8  [T N] episode ended after this step                  */
    double* ep_return;         /* f64 [N] open-episode return, persists across calls       */
    int32_t* ep_count;         /* i32 [N] episodes finished in this call                   */
    double* ep_sum_return;     /* f64 [N]                                                  */
    int32_t* ep_sum_length;    /* i32 [N]                                                  */
    int32_t* ep_successes;     /* i32 [N] finished episodes that terminated (>= 3 contacts) */
    int32_t diag_flags;        /* diagnostics only (timing ablations): bit0 skip the actor MLP
                                  (mu = 0), bit1 skip the env step; kernel selection (bit-
                                  identical tapes): 16 the one-lane-per-env kernel, 1024 the
                                  32-env kernel (default at >= 32 envs per CU), 2048 the 16-env
                                  kernel at any size; 128 per-step cycle stamps of the 16- / 32-env
                                  kernel (printed to stderr); 256 skip the 16-env kernel's draws,
                                  512 its reward settle (timing only: results are wrong); 32 / 64
                                  (the retired 4-wave kernel) are rejected; 0 in every real run */
    int32_t success_rule;      /* DXRL_SUCCESS_* for the episode records                   */
    int32_t record_cap;        /* per-env episode records [N][record_cap] (0 = none)       */
    double* rec_return;
    int32_t* rec_length;
    uint8_t* rec_success;
    int32_t* rec_end_step;     /* step index t within this call                            */
    uint16_t* ep_code;         /* u16 [T N] episode-end codes for the curriculum scheduler feed
                                  (dxrl_sched_scan): 0 = no episode ended at this step, else
                                  (episode length << 1) | success (nullable)                  */
    float* applied_act;        /* f32 [T N][16] the action the env integrated, after dynamics
                                  noise (nullable; parity checks replay it on the CPU)        */
    /* Fused-noise tapes (config C5; nullable, parity checks only; default kernel only): the
       f32 noise values exactly as the kernel added them, n = f32(sigma) * z with z the
       device's Box-Muller normal -- robustness_tests.py:180-182 draws n = N(0, sigma) and
       adds f32(n) to the action; :199-207 adds f32(n) to every observation element. */
    float* dyn_noise_tape;     /* f32 [T N][16] dynamics noise per action dim (0 if off)    */
    float* obs_noise_tape;     /* f32 [(T+1) N][48] observation noise per obs element       */
    void* h2_tape;             /* bf16 [T N][264] the actor's layer-2 activations of every step
                                  (nullable; written by the 16- and 32-env kernels, not the 64-env
                                  reference one, see dxrl_pg_rollout_kernel;
                                  dxrl_pg_fused_args.h2_in of the actor's first train pass under
                                  these weights)                                               */
} dxrl_pg_rollout_args;

/* Fused policy + env rollout: T steps of actor MLP (bf16 MFMA) -> Gaussian
 * sample -> [dynamics noise] -> env step -> tape, auto-reset (device RNG).
 * The reward follows the env's config (reward_type): the dense shaped reward, or the sparse one of
 * rewards/reward_shaping.py:228-234 (1.0 on a step with >= 3 contacts, -0.01 otherwise), which
 * leaves the env's previous-contact bits alone, as dxrl_env_step does. */
int dxrl_pg_rollout(dxrl_env* env, const void* packed, const float* params, const dxrl_pg_rollout_args* args,
                    void* stream);
/* Which kernel dxrl_pg_rollout runs for this env and diag_flags (without a feature-major tape):
 * 1 the 16-env kernel (< 32 envs per CU), 2 the 32-env kernel (both write h2_tape),
 * 0 the 64-env reference kernel (diag_flags & 16).  Host-only query. */
int dxrl_pg_rollout_kernel(const dxrl_env* env, int32_t diag_flags, int32_t* kernel);

/* GAE reverse scan; values f32 [(T+1) N]; writes adv/ret [T N] and this rank's advantage
 * moments stats[5] = T N, stats[6] = mean(adv), stats[7] = sum of squared deviations, and
 * stats[0..4] as dxrl_pg_adv_combine(stats + 5, world = 1) would (single rank: no second call)
 * (per-env sums about the env's own first value, merged with Chan et al.'s pairwise update
 * in a fixed order: no sum(a^2) - mean sum(a) cancellation).
 * The recurrence is A_t = delta_t + (gamma lambda)(1 - d_t) A_{t+1} per env:
 *   T <= 600 (~256 B per step in LDS, <= 152 KiB): k_gae_lds -- a 256-thread workgroup per 16
 *     envs stages the horizon in LDS with all its threads (delta_t and the chain coefficient
 *     computed in parallel), runs the recurrence as a wavefront-prefix scan (16 lanes per env:
 *     each lane's segment of 8-step chunks composed into an affine map, a suffix scan of the maps
 *     across the 16 lanes, each segment rerun from its incoming value), all threads store
 *     adv / ret; ceil(N / 16) workgroups.  Bit-exact against tests/pg_reference.py's restatement
 *     of that order; within ~1e-6 of the values' scale of the one-chain loop;
 *   longer horizons: k_gae -- one thread per env running the sequential loop, 64-env workgroups;
 *     ceil(N / 64) workgroups.
 * Each workgroup writes one (count, mean, M2) triple into `partial`.
 * partial: f64 [dxrl_pg_gae_partial_doubles(N, T)] (= 3 ceil(N / 16), enough for either kernel);
 * stats: f64 [8]. */
int dxrl_pg_gae(int32_t device, const float* rew, const uint8_t* done, const float* values, int64_t num_envs,
                int64_t horizon, double gamma, double lam, float* adv, float* ret, double* partial, double* stats,
                void* stream);
/* f64 elements of dxrl_pg_gae's `partial` scratch for (num_envs, horizon) (host-only query). */
int dxrl_pg_gae_partial_doubles(int64_t num_envs, int64_t horizon, int64_t* doubles);
/* dxrl_pg_gae with the time-limit bootstrap: the tape is the rollout's episode-end code ep_code
 * u16 [T N] (dxrl_pg_rollout_args.ep_code under success_rule "terminated": 0, or
 * (episode length << 1) | terminated) in place of the done byte.  Per sample, in f32, in this order:
 *   end = code != 0, term = code & 1, timeout = end && !term
 *   vb = timeout ? V_t : V_{t+1};  nb = term ? 0 : 1
 *   delta_t = r_t + gamma vb nb - V_t;  c_t = end ? 0 : gamma lambda
 *   A_t = delta_t + c_t A_{t+1};  ret_t = A_t + V_t
 * The chain stops at either kind of end; a termination drops the bootstrap as dxrl_pg_gae does at
 * every done, an end at the run_episode loop bound (a time limit, not a property of the state)
 * keeps it.  The state the bootstrap belongs to, the one the episode's last step led to, is
 * overwritten by the reset and not on the tape: V_t, the critic's value of the state the last
 * action was taken in, stands in for it.  That is an approximation (the states are one first-order
 * dynamics step apart), not the exact time-limit bootstrap.
 * Kernels (chosen by horizon as in dxrl_pg_gae, DXRL_GAE_SEQ included), scans, moments, `partial`
 * (dxrl_pg_gae_partial_doubles) and stats[0..7] are dxrl_pg_gae's; two launches.  On a tape whose
 * codes all have bit 0 set, adv / ret are dxrl_pg_gae's on done = code != 0, bit for bit.
 * counts: i64 [dxrl_pg_gae_timelimit_count_words(N, T)]: counts[0] = time limits, counts[1] =
 * terminations on the tape -- exact: integer sums of the launched workgroups' (time limits,
 * terminations) pairs, which follow from counts[2] on (16 envs per pair in k_gae_lds, 64 in k_gae).
 * DXRL_E_INVALID before any launch on a null pointer or num_envs / horizon < 1. */
int dxrl_pg_gae_timelimit(int32_t device, const float* rew, const uint16_t* ep_code, const float* values,
                          int64_t num_envs, int64_t horizon, double gamma, double lam, float* adv, float* ret,
                          double* partial, double* stats, int64_t* counts, void* stream);
/* i64 elements of dxrl_pg_gae_timelimit's `counts` for (num_envs, horizon) (= 2 + 2 ceil(N / 16);
 * host-only query). */
int dxrl_pg_gae_timelimit_count_words(int64_t num_envs, int64_t horizon, int64_t* words);

/* ---- value normalisation: running return moments in the advantages phase ----------------
 * The critic works in normalised units; dxrl_pg_gae_vnorm decodes its outputs and encodes its
 * targets with the running mean / standard deviation of all raw returns seen so far.
 *
 * State: vnorm, f64 [DXRL_PG_VNORM_WORDS] on the device (enum below).  A fresh block is all zero
 * except DXRL_PG_VNORM_MU = 0 and DXRL_PG_VNORM_SIGMA = 1.
 *
 * One call under the block's (mu, sigma), both read from the block as f32; all arithmetic f32, in
 * this order, nothing fused:
 *   v_t    = sigma * vn_t + mu             for all (T + 1) N critic outputs vn (`values`)
 *   adv, ret = dxrl_pg_gae (done) or dxrl_pg_gae_timelimit (ep_code) on (rew, tape, v)
 *   retn_t = (ret_t - mu) / sigma          a true, correctly rounded f32 division (the library is
 *                                          built with correctly rounded division; no stored 1 / sigma)
 * Outputs: adv, ret [T N] raw, as those two write them; ret_norm [T N] = retn, what the critic's
 * train pass regresses; values_raw [(T + 1) N] = v; stats[0..7] as dxrl_pg_gae; counts as
 * dxrl_pg_gae_timelimit (ep_code only).  Under a fresh block v = 1 * vn + 0 and retn = ret: the
 * call's adv / ret / stats are the plain entry's bit for bit on values without a -0.0 (which
 * decodes to +0.0).
 * Then the fold.  The call's return triple (count, mean, M2 of ret) is reduced as the advantage
 * triple is -- shifted f64 sums per thread, the workgroup's fixed merge tree, one finishing
 * workgroup over the partials in the same order -- and written to BATCH_*; stats[5..7] is copied
 * to ADV_* directly behind it (six contiguous doubles: what ranks exchange).  With fold != 0 the
 * batch triple is merged into the running triple (dxrl::merge(running, batch)), CALLS grows by
 * one, and the constants of the NEXT call are refreshed (only when the running count is > 0):
 *   mu = (float)mean;  sigma = (float)sqrt(M2 / count + eps)     (f64 arithmetic, then narrowed)
 * so within one call the same (mu, sigma) decode the critic and encode its targets, and the
 * state lags the data by exactly one call.  eps is stored in the block for dxrl_pg_vnorm_combine.
 * Forgetting: every fold (here and in dxrl_pg_vnorm_combine) first discounts the running triple
 * with d = 1 - FORGET (f64): count <- d count, M2 <- d M2, the mean kept; then the merge and the
 * refresh above.  FORGET = 0 (a fresh block) gives d = 1 and the pooled moments, bit for bit;
 * with FORGET > 0 the count settles near batch count / FORGET, so late returns keep their weight.
 * eps = 0 with constant returns gives sigma = 0: the caller's choice.
 * Launches: two, as the plain entries (the kernel chosen by horizon as in dxrl_pg_gae,
 * DXRL_GAE_SEQ included, in its value-normalisation instantiation; then one finishing launch).
 * partial: f64 [dxrl_pg_gae_vnorm_partial_doubles(N, T)]: the workgroups' advantage triples, then
 * their return triples.
 * DXRL_E_INVALID before any launch, outputs untouched: a null pointer (counts may be null with
 * `done`), both tapes or neither, num_envs or horizon < 1, eps < 0. */
enum dxrl_pg_vnorm_word {
    DXRL_PG_VNORM_COUNT = 0,    /* running triple of all raw returns folded so far          */
    DXRL_PG_VNORM_MEAN,
    DXRL_PG_VNORM_M2,
    DXRL_PG_VNORM_MU,           /* f32 constants of the next call, widened to f64           */
    DXRL_PG_VNORM_SIGMA,
    DXRL_PG_VNORM_BATCH_COUNT,  /* the last call's return triple                            */
    DXRL_PG_VNORM_BATCH_MEAN,
    DXRL_PG_VNORM_BATCH_M2,
    DXRL_PG_VNORM_ADV_COUNT,    /* copy of the last call's stats[5..7] (after a combine:    */
    DXRL_PG_VNORM_ADV_MEAN,     /* the ranks' merged advantage triple)                      */
    DXRL_PG_VNORM_ADV_M2,
    DXRL_PG_VNORM_CALLS,        /* batches folded                                           */
    DXRL_PG_VNORM_EPS,          /* eps of the last dxrl_pg_gae_vnorm call                   */
    DXRL_PG_VNORM_FORGET,       /* forgetting factor of the fold, in [0, 1): set by the owner
                                   of the block before the first call, written by no entry  */
    DXRL_PG_VNORM_NAMED
};
#define DXRL_PG_VNORM_WORDS 16  /* words from DXRL_PG_VNORM_NAMED on are zero */
typedef struct dxrl_pg_gae_vnorm_args {
    const float* rew;           /* f32 [T N]                                                */
    const uint8_t* done;        /* u8 [T N]: the done-byte rule (dxrl_pg_gae), or NULL      */
    const uint16_t* ep_code;    /* u16 [T N]: the time-limit rule (dxrl_pg_gae_timelimit), or NULL */
    const float* values;        /* f32 [(T + 1) N] critic outputs, normalised units         */
    int64_t num_envs, horizon;
    double gamma, lam, eps;
    float* adv;                 /* f32 [T N] raw advantages                                 */
    float* ret;                 /* f32 [T N] raw returns                                    */
    float* ret_norm;            /* f32 [T N] (ret - mu) / sigma                             */
    float* values_raw;          /* f32 [(T + 1) N] sigma values + mu                        */
    double* partial;            /* f64 [dxrl_pg_gae_vnorm_partial_doubles(N, T)]            */
    double* stats;              /* f64 [8]                                                  */
    int64_t* counts;            /* ep_code: i64 [dxrl_pg_gae_timelimit_count_words(N, T)]   */
    double* vnorm;              /* f64 [DXRL_PG_VNORM_WORDS]                                */
    int32_t fold;               /* 0: write BATCH_* / ADV_* / EPS only (a rank of a sharded
                                   trainer; dxrl_pg_vnorm_combine folds)                    */
} dxrl_pg_gae_vnorm_args;
int dxrl_pg_gae_vnorm(int32_t device, const dxrl_pg_gae_vnorm_args* args, void* stream);
/* f64 elements of dxrl_pg_gae_vnorm's `partial` for (num_envs, horizon) (= 6 ceil(N / 16);
 * host-only query). */
int dxrl_pg_gae_vnorm_partial_doubles(int64_t num_envs, int64_t horizon, int64_t* doubles);
/* Sharded trainers: moments6 f64 [world][6] in rank order, each row a rank's BATCH_* and ADV_*
 * words after its own dxrl_pg_gae_vnorm call with fold = 0 (one all-gather).  Writes stats[0..4]
 * exactly as dxrl_pg_adv_combine would from the rows' advantage triples; merges the return
 * triples in rank order (from the empty triple) into BATCH_*, writes the merged advantage triple
 * to ADV_*, and folds BATCH_* into the running state as dxrl_pg_gae_vnorm does with fold != 0,
 * with the block's EPS.  EPS is the word the last dxrl_pg_gae_vnorm call on the block wrote (eps
 * is an argument of that call alone): a combine on a fresh block, with no such call before it, folds with
 * eps = 0, so a caller that combines hand-made rows writes DXRL_PG_VNORM_EPS itself first.  Every
 * rank ends with the same state bytes; with world = 1 they are the bytes fold = 1 leaves.  One
 * launch. */
int dxrl_pg_vnorm_combine(int32_t device, const double* moments6, int32_t world, double* stats, double* vnorm,
                          void* stream);

/* ---- PopArt: keep the critic's decoded values when (mu, sigma) move --------------------------
 * The critic's head (kOffW3c row 0: 256 weights, then the bias in column 256) puts out values in
 * the units of some pair (mu_h, sigma_h); dxrl_pg_gae_vnorm decodes them with the vnorm block's
 * (MU, SIGMA) = (mu_n, sigma_n).  dxrl_pg_popart_rescale rewrites the head so that it puts out the
 * units of (mu_n, sigma_n) and decodes to what it decoded to before.
 *
 * State: popart, f64 [DXRL_PG_POPART_WORDS] on the device (enum below).  A fresh block is all zero
 * except DXRL_PG_POPART_SIGMA_HEAD = 1.  The vnorm block is only read.
 *
 * Arithmetic: all f64, nothing fused, one rounding to f32 per stored value.
 *   s  = sigma_h / sigma_n
 *   w' = (float)((double)w * s)                                       the 256 head weights
 *   b' = (float)((sigma_h * (double)b + (mu_h - mu_n)) / sigma_n)     the bias
 *   MU_HEAD = mu_n; SIGMA_HEAD = sigma_n; RESCALES += 1; LAST_SCALE = s;
 *   LAST_SHIFT = (mu_h - mu_n) / sigma_n
 * so sigma_n (w' h + b') + mu_n = sigma_h (w h + b) + mu_h up to the f32 roundings of w', b'.
 * Written: the 257 master floats in place in `params`, and every copy of them in the bf16 `packed`
 * buffer (the pack then equals dxrl_pg_pack_weights(params) byte for byte).  Nothing else of
 * either buffer changes.  Adam's moments of the head are NOT rescaled (PopArt's own choice: they
 * keep describing gradients in the old units and decay at Adam's rates).
 * The cases, decided in this order:
 *   refusal: sigma_h or sigma_n not finite or <= 0, or mu_h or mu_n not finite (eps = 0 on constant
 *            returns gives sigma_n = 0): SKIPPED += 1 and nothing else is written, row_out included;
 *   no-op:   (mu_h, sigma_h) equal (mu_n, sigma_n) bitwise: params, packed and the block stay
 *            untouched (a call on a fresh pair rounds nothing); row_out is written with
 *            rescaled = 0, scale = 1, shift = 0;
 *   rescale: the above; row_out is written with rescaled = 1.
 * The entry keeps no order of its own: it compares the two blocks, so it may run after any
 * iteration, updated or not, resumed or not.
 * row_out: f64 [DXRL_PG_VNORM_LOG_COLS] or NULL (enum below), written by the same launch; std =
 * sqrt(M2 / count) (0 for an empty triple).
 * One launch of one workgroup.  DXRL_E_INVALID before any launch for a null params / packed /
 * vnorm / popart. */
enum dxrl_pg_popart_word {
    DXRL_PG_POPART_MU_HEAD = 0,  /* the units the critic's head puts out                     */
    DXRL_PG_POPART_SIGMA_HEAD,
    DXRL_PG_POPART_RESCALES,     /* calls that changed the head                              */
    DXRL_PG_POPART_SKIPPED,      /* calls refused on the device                              */
    DXRL_PG_POPART_LAST_SCALE,   /* s and the shift of the last rescale                      */
    DXRL_PG_POPART_LAST_SHIFT,
    DXRL_PG_POPART_NAMED
};
#define DXRL_PG_POPART_WORDS 8   /* words from DXRL_PG_POPART_NAMED on are zero */
enum dxrl_pg_vnorm_log_col {     /* the row of an iteration, f64 [DXRL_PG_VNORM_LOG_COLS]    */
    DXRL_PG_VNORM_LOG_MU = 0,    /* the pair the next iteration decodes with, = the head's   */
    DXRL_PG_VNORM_LOG_SIGMA,
    DXRL_PG_VNORM_LOG_MU_PREV,   /* the head's pair before the call                          */
    DXRL_PG_VNORM_LOG_SIGMA_PREV,
    DXRL_PG_VNORM_LOG_SCALE,     /* s (1 on the no-op path)                                  */
    DXRL_PG_VNORM_LOG_SHIFT,     /* (mu_prev - mu) / sigma (0 on the no-op path)             */
    DXRL_PG_VNORM_LOG_RESCALED,  /* 0 / 1                                                    */
    DXRL_PG_VNORM_LOG_COUNT,     /* the running triple, as count / mean / std                */
    DXRL_PG_VNORM_LOG_MEAN,
    DXRL_PG_VNORM_LOG_STD,
    DXRL_PG_VNORM_LOG_BATCH_MEAN,
    DXRL_PG_VNORM_LOG_BATCH_STD,
    DXRL_PG_VNORM_LOG_CALLS,
    DXRL_PG_VNORM_LOG_FORGET,
    DXRL_PG_VNORM_LOG_COLS
};
typedef struct dxrl_pg_popart_args {
    float* params;               /* f32 master [dxrl_pg_sizes params]                        */
    void* packed;                /* bf16 pack [dxrl_pg_sizes packed_bf16]                    */
    const double* vnorm;         /* f64 [DXRL_PG_VNORM_WORDS], read                          */
    double* popart;              /* f64 [DXRL_PG_POPART_WORDS]                               */
    double* row_out;             /* f64 [DXRL_PG_VNORM_LOG_COLS] or NULL                     */
} dxrl_pg_popart_args;
int dxrl_pg_popart_rescale(int32_t device, const dxrl_pg_popart_args* args, void* stream);
/* Global advantage statistics from every rank's (count, mean, M2) triple -- moments f64
 * [world][3] in rank order (all-gathered stats[5..7]) -- merged in rank order into
 * stats[0] count, [1] sum, [2] mean, [3] sum of squared deviations, [4] unbiased std (what the
 * train passes read: (adv - [2]) / ([4] + 1e-8)). */
int dxrl_pg_adv_combine(int32_t device, const double* moments, int32_t world, double* stats, void* stream);
/* One rank: dxrl_pg_adv_combine(stats + 5, world = 1).  phase must be 2; adv / count /
 * partial are unused (kept for ABI stability). */
int dxrl_pg_adv_finalize(int32_t device, int32_t phase, const float* adv, int64_t count, double* partial,
                         double* stats, void* stream);

/* ------------------------------------------------------------------------
 * Curriculum-scheduler feed (config C3; replaces the per-episode
 * CurriculumScheduler.update() calls of evaluation/component_ablation.py:160-170,
 * experiments/curriculum_scheduler.py:116-170 for a vectorised iteration).
 * Walks the rollout's episode-end codes (dxrl_pg_rollout_args.ep_code) of all
 * ranks in (end step, global env id) order and reports what the host scheduler
 * needs to replay the batch exactly.
 * ------------------------------------------------------------------------ */
#define DXRL_SCHED_MAX_CANDIDATES 64
typedef struct dxrl_sched_args {
    const uint16_t* codes;     /* u16 [world][T][N] episode-end codes, rank-major (all-gathered) */
    int32_t world, horizon;    /* ranks, T                                                 */
    int64_t num_envs;          /* N per rank                                               */
    int32_t window;            /* window_size (>= 1)                                       */
    int32_t max_candidates;    /* P <= DXRL_SCHED_MAX_CANDIDATES progressions still possible */
    double threshold;          /* success_rate_threshold                                   */
    int64_t min_episodes;      /* min_episodes_before_progression                          */
    int64_t episodes_before;   /* total_episodes before this batch (== len(episode_successes)) */
    const uint16_t* tail_in;   /* u16 [window] codes of the last tail_len_in episodes, oldest first */
    const int32_t* tail_len_in;   /* i32 [1] (device)                                      */
    uint16_t* tail_out;        /* u16 [window] the new tail (must not alias tail_in)       */
    int32_t* tail_len_out;     /* i32 [1] (device)                                         */
    void* scratch;             /* device scratch of dxrl_sched_scratch_bytes()             */
    int64_t scratch_bytes;
    int64_t* summary;          /* i64 [4 + 3 P] (device): [0] episodes, [1] steps, [2] successes,
                                  [3] candidates found (<= P), then per candidate in episode order:
                                  episode index k in the batch, steps through k, successes among
                                  the window ending at k                                        */
} dxrl_sched_args;
int dxrl_sched_scratch_bytes(int32_t world, int32_t horizon, int64_t num_envs, int32_t window, int64_t* bytes);
int dxrl_sched_scan(int32_t device, const dxrl_sched_args* args, void* stream);

/* The same feed with a compacted exchange between ranks (what a sharded run all-gathers instead
 * of the world x T x N codes).  Each rank packs its own codes [T][N]:
 *   header (episodes, tail length), per-step (episodes, steps, successes), its last `window`
 *   codes, and -- only while progressions are still possible (bits = 1) -- one success bit
 *   per episode;
 * = 4 (2 + 3 T + window / 2) bytes, + T N / 8 with bits.  The ranks all-gather the packs,
 * dxrl_sched_scan_packed walks them in (end step, global env id) order exactly as
 * dxrl_sched_scan walks the codes, and reports every candidate's steps only through the start
 * of its (step, rank) block plus where it lies (`where`); the owning rank adds the steps inside
 * the block (dxrl_sched_candidate_steps -> i64 [P], zero for others), the ranks SUM those P
 * values (all-reduce) and dxrl_sched_finish adds them into the summary.  The summary / tail
 * equal dxrl_sched_scan's on the all-gathered codes. */
int dxrl_sched_pack_words(int32_t horizon, int64_t num_envs, int32_t window, int32_t bits, int64_t* words);
int dxrl_sched_pack(int32_t device, const uint16_t* codes, int32_t horizon, int64_t num_envs, int32_t window,
                    int32_t bits, uint32_t* pack, void* stream);
typedef struct dxrl_sched_packed_args {
    const void* packs;         /* u32 [world][pack_words] all-gathered packs, rank order  */
    int64_t pack_words;        /* dxrl_sched_pack_words(horizon, num_envs, window, bits)  */
    int32_t bits;              /* the packs carry success bits (needed when max_candidates > 0) */
    int32_t world, horizon;
    int64_t num_envs;          /* N per rank                                              */
    int32_t window, max_candidates;
    double threshold;
    int64_t min_episodes, episodes_before;
    const uint16_t* tail_in;   /* as dxrl_sched_args                                      */
    const int32_t* tail_len_in;
    uint16_t* tail_out;
    int32_t* tail_len_out;
    void* scratch;             /* dxrl_sched_packed_scratch_bytes()                       */
    int64_t scratch_bytes;
    int64_t* summary;          /* as dxrl_sched_args (candidate steps: block prefix until finished) */
    int32_t* where;            /* i32 [P][3] per candidate: owning rank, end step, index in its block */
} dxrl_sched_packed_args;
int dxrl_sched_packed_scratch_bytes(int32_t world, int32_t horizon, int64_t num_envs, int32_t window,
                                    int64_t* bytes);
int dxrl_sched_scan_packed(int32_t device, const dxrl_sched_packed_args* args, void* stream);
int dxrl_sched_candidate_steps(int32_t device, const uint16_t* codes, int32_t horizon, int64_t num_envs,
                               int32_t rank, int32_t max_candidates, const int32_t* where, const int64_t* summary,
                               int64_t* partial, void* stream);
int dxrl_sched_finish(int32_t device, const int64_t* partial, int64_t* summary, void* stream);

typedef struct dxrl_pg_heads_args {
    const float* mu;           /* f32 [M][32] actor head output            */
    const float* values;       /* f32 [M] critic value                     */
    const float* act;          /* f32 [M][16]                              */
    const float* logp_old;     /* f32 [M]                                  */
    const float* adv;          /* f32 [M] raw GAE advantages               */
    const float* ret;          /* f32 [M] returns                          */
    const double* stats;       /* normalisation stats (mean [2], std [4])  */
    const float* params;       /* f32 master parameters (log_std)          */
    int64_t num_samples;       /* M (this rank)                            */
    double inv_total_samples;  /* 1 / (M summed over ranks)                */
    double clip_eps, vf_coef, ent_coef;
    void* dmu_rm;              /* bf16 [M][32]                             */
    void* dmu_fm;              /* bf16 [32][M]                             */
    void* dv_rm;               /* bf16 [M][32] (column 0)                  */
    void* dv_fm;               /* bf16 [32][M] (row 0)                     */
    float* dlogstd_partial;    /* f32 [ceil(M/256)][16]                    */
    double* loss_partial;      /* f64 [ceil(M/256)][4]                     */
    float* grads;              /* f32 master-layout gradients (log_std block written) */
} dxrl_pg_heads_args;

/* PPO-clip policy loss + value loss + entropy bonus: gradients at the heads. */
int dxrl_pg_heads(int32_t device, const dxrl_pg_heads_args* args, void* stream);
/* out[0] = sum(grads^2) (for global-norm clipping; all-reduce before Adam when sharded). */
int dxrl_pg_grad_sumsq(int32_t device, const float* grads, int64_t n, double* partial, double* out, void* stream);
int dxrl_pg_adam(int32_t device, float* params, const float* grads, float* m1, float* m2, int64_t n, double lr,
                 double beta1, double beta2, double eps, int64_t step, const double* gnorm2, double max_norm,
                 void* stream);
/* The whole optimiser step in two launches: grad-norm partials, then one kernel that finishes
 * the norm (k_sum_partials' order), applies clipped Adam (dxrl_pg_adam's arithmetic) and writes
 * the bf16 pack (dxrl_pg_pack_weights' layout) -- the updated master / moments go to the *_out
 * buffers (must not alias the inputs; the caller swaps the pairs).  n = dxrl_pg_sizes().params;
 * partial: f64 [512] scratch; gnorm2: f64 [1] (sum of squared grads, written). */
int dxrl_pg_optimizer_step(int32_t device, const float* params, const float* grads, const float* m1, const float* m2,
                           float* params_out, float* m1_out, float* m2_out, int64_t n, double lr, double beta1,
                           double beta2, double eps, int64_t step, double max_norm, double* partial, double* gnorm2,
                           void* packed, void* stream);
/* dxrl_pg_optimizer_step's second launch alone: the grad norm is finished from gnorm_blocks f64
 * partials the caller already holds (dxrl_pg_fused_pair_gnorm's, when one rank's reduction wrote
 * the whole gradient) instead of a k_sumsq pass over the gradient.  Same Adam / pack arithmetic;
 * the norm's f64 sum runs in another order, so it agrees with dxrl_pg_optimizer_step's to f64
 * rounding, not bit for bit.  New learner, no reference counterpart. */
int dxrl_pg_adam_step(int32_t device, const float* params, const float* grads, const float* m1, const float* m2,
                      float* params_out, float* m1_out, float* m2_out, int64_t n, double lr, double beta1, double beta2,
                      double eps, int64_t step, double max_norm, const double* gnorm_partial, int32_t gnorm_blocks,
                      double* gnorm2, void* packed, void* stream);

/* ---- step-size control on the device (PPO: LR schedule, KL stop, KL-adaptive LR) --------
 * dxrl_pg_adam_step_ctl is dxrl_pg_adam_step / dxrl_pg_optimizer_step with the learning rate,
 * Adam's t and whether the pass is applied at all decided inside the one optimiser launch, from
 * the pass's approx-KL sums (column 3 of the learner's loss partials) and a device state block.
 * No reference counterpart (policies/simple_learner.py has one fixed learning rate).
 *
 * State: 2 slots of DXRL_PG_OPT_SLOT_WORDS 64-bit words (int64 or f64 per slot enum below).  Call
 * number c (ctl.calls, 1-based, the host's count) reads slot (c - 1) & 1 and writes slot c & 1.
 * A fresh block: all zero but DXRL_PG_OPT_SCALE = 1.0 and DXRL_PG_OPT_STOP_PASS = -1 in slot 0.
 *
 * Pass u of an iteration, kl = (sum of column 3) / pass_rows:
 *   pass_index == 0 clears the iteration's stop flag and accumulators;
 *   target_kl > 0, not yet stopped and kl > stop_factor * target_kl (strict): stopped at u;
 *   stopped: *_out = inputs bit for bit, pack untouched, the pass counts as skipped;
 *   else lr = clamp(lr_nominal * scale, lr_min, lr_max) (f64, then f32), Adam with
 *   t = applied + 1 (skipped passes do not advance t; while no pass was ever skipped the bias
 *   corrections are the host's for t = calls, dxrl_pg_adam_step's bytes; afterwards
 *   1 - pow(beta, t) in f64 on the device);
 *   last_epoch passes add (KL sum, pass_rows) to the epoch accumulators, applied or not;
 *   last_pass: kl_epoch = accumulated sum / rows (0 with no rows); with adapt and target_kl > 0:
 *   kl_epoch > adapt_band * target_kl: scale /= adapt_factor, else kl_epoch < target_kl /
 *   adapt_band: scale *= adapt_factor; scale is then moved so that lr_nominal * scale is inside
 *   [lr_min, lr_max]; the row (enum dxrl_pg_opt_col) is written to row_out when it is non-null.
 * The new scale holds from the next call on.  gnorm2 is written by every call. */
typedef struct dxrl_pg_lr_control {
    double lr_nominal, lr_min, lr_max;
    double target_kl;      /* 0: no KL rule                                     */
    double stop_factor;    /* +inf: adapt without stopping                      */
    double adapt_factor, adapt_band;
    int32_t adapt;         /* 0 / 1                                             */
    int32_t pass_index;    /* within the iteration                              */
    int32_t last_epoch;    /* 0 / 1: a pass of the iteration's last epoch       */
    int32_t last_pass;     /* 0 / 1: the iteration's last pass                  */
    int64_t calls;         /* the host's call count, this call included (>= 1)  */
} dxrl_pg_lr_control;

enum dxrl_pg_opt_slot {
    DXRL_PG_OPT_APPLIED = 0,      /* i64 passes applied so far (Adam's t)            */
    DXRL_PG_OPT_SKIPPED,          /* i64 passes skipped so far                       */
    DXRL_PG_OPT_SCALE,            /* f64 the KL-adaptive factor on lr_nominal        */
    DXRL_PG_OPT_STOPPED,          /* i64 0 / 1: this iteration is stopped            */
    DXRL_PG_OPT_STOP_PASS,        /* i64 the pass it stopped at, -1: none            */
    DXRL_PG_OPT_ITER_APPLIED,     /* i64 passes applied in this iteration            */
    DXRL_PG_OPT_ITER_SKIPPED,     /* i64 passes skipped in this iteration            */
    DXRL_PG_OPT_LR_FIRST,         /* f64 lr of the iteration's first applied pass, 0 */
    DXRL_PG_OPT_LR_LAST,          /* f64 lr of its last applied pass, 0              */
    DXRL_PG_OPT_KL_MAX,           /* f64 largest pass KL of the iteration            */
    DXRL_PG_OPT_KL_SUM,           /* f64 KL sums of the last epoch's passes          */
    DXRL_PG_OPT_KL_ROWS,          /* f64 samples of the last epoch's passes          */
    DXRL_PG_OPT_NAMED
};
#define DXRL_PG_OPT_SLOT_WORDS 16
#define DXRL_PG_OPT_STATE_WORDS (2 * DXRL_PG_OPT_SLOT_WORDS)

enum dxrl_pg_opt_col {            /* the row of an iteration, f64 [DXRL_PG_OPT_COLS] */
    DXRL_PG_OPT_COL_LR = 0,       /* lr of the first applied pass (0: none applied)  */
    DXRL_PG_OPT_COL_LR_LAST,      /* lr of the last applied pass                     */
    DXRL_PG_OPT_COL_UPDATES,      /* passes applied                                  */
    DXRL_PG_OPT_COL_SKIPPED,      /* passes skipped                                  */
    DXRL_PG_OPT_COL_STOP_PASS,    /* -1: no stop                                     */
    DXRL_PG_OPT_COL_KL_MAX,
    DXRL_PG_OPT_COL_KL_EPOCH,
    DXRL_PG_OPT_COL_LR_SCALE,     /* the scale of the next iteration                 */
    DXRL_PG_OPT_COLS
};

/* gnorm_blocks > 0: gnorm_partial holds that many f64 partials of the squared grad norm
 * (dxrl_pg_fused_pair_gnorm's); gnorm_blocks == 0: gnorm_partial is f64 [512] scratch that a
 * k_sumsq launch fills first, as in dxrl_pg_optimizer_step.  loss_partial: f64 [loss_blocks][4];
 * state: [DXRL_PG_OPT_STATE_WORDS]; row_out: f64 [DXRL_PG_OPT_COLS] or NULL. */
int dxrl_pg_adam_step_ctl(int32_t device, const float* params, const float* grads, const float* m1, const float* m2,
                          float* params_out, float* m1_out, float* m2_out, int64_t n, double beta1, double beta2,
                          double eps, double max_norm, double* gnorm_partial, int32_t gnorm_blocks, double* gnorm2,
                          void* packed, const double* loss_partial, int32_t loss_blocks, int64_t pass_rows,
                          dxrl_pg_lr_control ctl, int64_t* state, double* row_out, void* stream);

/* ---- step-size control on sharded trainers: one KL record per rank ---------------------
 * Each rank of a sharded trainer sees the KL of its own shard only; ranks on opposite sides of a
 * threshold would apply different updates.  So every rank packs (kl_sum, rows) of its pass into a
 * record, the records are all-gathered in rank order, and every rank merges the same bytes in the
 * same order inside its optimiser launch: the same decision on every rank.
 *
 * Convention: column 3 of the loss partials holds UNSCALED sums of (logp_old - logp) over the
 * rank's own samples -- neither dxrl_pg_fused nor dxrl_pg_heads applies inv_total_samples (which
 * carries the world factor 1 / (rows x world) on a sharded trainer) to the loss columns, only to
 * the gradients -- and pass_rows counts the rank's own samples.  A record therefore holds a plain
 * sum and a plain count, and the merged kl = sum_r kl_sum_r / sum_r rows_r is the mean approximate
 * KL over the samples of all ranks, for equal and unequal shards alike.
 *
 * dxrl_pg_kl_rank_pack: one launch of one workgroup.  record[0] = the sum of column 3 of
 * loss_partial (f64 [loss_blocks][4]) in exactly the order dxrl_pg_adam_step_ctl sums it;
 * record[1] = (double)pass_rows.  Null pointers, loss_blocks < 1 or pass_rows < 1 are refused with
 * the record untouched. */
#define DXRL_PG_KL_RECORD_WORDS 2
int dxrl_pg_kl_rank_pack(int32_t device, const double* loss_partial, int32_t loss_blocks, int64_t pass_rows,
                         double* record, void* stream);

/* dxrl_pg_adam_step_ctl with (loss_partial, loss_blocks, pass_rows) replaced by the gathered
 * records: f64 [world][DXRL_PG_KL_RECORD_WORDS] in rank order, world >= 1.  Every workgroup reads
 * the 2 x world doubles and merges them sequentially in rank order, kl_sum = ((r0 + r1) + r2) ..
 * and rows likewise; everything after that is dxrl_pg_adam_step_ctl's rules, stated once.  With
 * world == 1 and the record dxrl_pg_kl_rank_pack wrote from the same partials the call writes
 * dxrl_pg_adam_step_ctl's bytes: *_out, pack, state slot, gnorm2 and row. */
int dxrl_pg_adam_step_ctl_world(int32_t device, const float* params, const float* grads, const float* m1,
                                const float* m2, float* params_out, float* m1_out, float* m2_out, int64_t n,
                                double beta1, double beta2, double eps, double max_norm, double* gnorm_partial,
                                int32_t gnorm_blocks, double* gnorm2, void* packed, const double* records,
                                int32_t world, dxrl_pg_lr_control ctl, int64_t* state, double* row_out,
                                void* stream);

/* ---- fused one-pass learner step (csrc/dxrl_pg_fused.hip) ----------------------------
 * One launch per network replaces forward GEMMs + heads + backward GEMMs of the
 * layer-by-layer path (dxrl_gemm_bf16 / dxrl_pg_heads / dxrl_wgrad_bf16): per
 * 128-sample tile it runs the MLP forward, the PPO-clip (actor) or value (critic)
 * head and the backward pass out of LDS (db2 as fused column sums of dH2), then
 * dW2 = dH2^T H1 as one split-K contraction over dH2 (HBM).  H1 reaches it either
 * recomputed on chip from obs (h1_mode 0, rows % 32 == 0: no H1 traffic at all) or as
 * the h1 scratch copy this launch writes (h1_mode 1, or rows % 32 != 0).
 * train == 0 (critic only): forward pass writing values[rows] (GAE bootstrap pass). */
typedef struct dxrl_pg_fused_args {
    int32_t net;               /* 0 actor, 1 critic                                        */
    int32_t train;             /* 0 forward only (critic values), 1 forward + backward     */
    int64_t rows;              /* samples                                                  */
    const void* packed;        /* bf16 weight pack (dxrl_pg_pack_weights)                  */
    const float* params;       /* f32 master parameters (biases, log_std)                  */
    const void* obs;           /* bf16 [rows][64], column 45 = 1                           */
    const float* act;          /* actor: f32 [rows][16]                                    */
    const float* logp_old;     /* actor: f32 [rows]                                        */
    const float* adv;          /* actor: f32 [rows] raw GAE advantages                     */
    const float* ret;          /* critic: f32 [rows] returns                               */
    const double* stats;       /* actor: normalisation stats (mean [2], std [4])           */
    double inv_total_samples;  /* 1 / (samples summed over ranks)                          */
    double clip_eps, vf_coef, ent_coef;
    float* values;             /* forward mode: f32 [rows]                                 */
    void* h1;                  /* bf16 [rows][288] scratch (used by the H1 copy mode only)  */
    void* dh2;                 /* bf16 [rows][256] scratch                                 */
    float* partial;            /* f32 [grid + 17][dxrl_pg_fused_sizes().partial_floats]    */
    double* loss_partial;      /* f64 [grid][4]: actor writes 0,2,3, critic writes 1       */
    int32_t grid;              /* workgroups (one per CU: 256 on MI355X)                   */
    int32_t wgrad_splits;      /* split-K factor of the dW2 GEMM                           */
    float* wgrad_partial;      /* f32 [wgrad_splits + 16][256][288]                        */
    float* grads;              /* f32 master-layout gradients: W1/W2/W3 (+ log_std) blocks */
    int32_t h1_mode;           /* 0 recompute H1 for dW2 when rows % 32 == 0, 1 HBM copy    */
    /* Layer-2 activations computed once per weight version (round 6; both nullable):
       h2_out (forward mode): bf16 [rows][264] H2 of the critic, written by the values pass;
       h2_in (train mode): bf16 [rows][264] H2 of this net under the SAME weights -- the rollout's
       h2_tape for the actor, the values pass's h2_out for the critic -- read instead of
       recomputing layer 2 (bit-identical: same MFMA k order and tanh).  Columns 256..263 are
       padding (keep them finite, e.g. zero-initialised). */
    const void* h2_in;
    void* h2_out;
} dxrl_pg_fused_args;

int dxrl_pg_fused_sizes(int32_t* tile_rows, int64_t* partial_floats_per_block);
int dxrl_pg_fused(int32_t device, const dxrl_pg_fused_args* args, void* stream);
/* Both train passes of one learner step (a PPO minibatch, or the whole batch) with their
 * dW2 contractions in ONE k_wgrad_l1 launch (critic->wgrad_splits + actor->wgrad_splits
 * workgroups side by side) and every reduction of both networks in ONE launch.  Same
 * per-network arithmetic as two dxrl_pg_fused calls with those split counts; each pass needs
 * its own dh2 / partial / wgrad_partial buffers, h1_mode 0, rows % 32 == 0, splits > 16.
 * No reference counterpart (policies/simple_learner.py:73-95 is the update it replaces). */
int dxrl_pg_fused_pair(int32_t device, const dxrl_pg_fused_args* critic, const dxrl_pg_fused_args* actor,
                       void* stream);
/* dxrl_pg_fused_pair whose reduction also writes the global grad norm's partials: one f64 per
 * reduction block (*gnorm_blocks of them, dxrl_pg_gnorm_blocks(); gnorm_capacity >= that), each
 * the sum of squares of the gradient values the block stored.  The gradients are bit for bit
 * dxrl_pg_fused_pair's.  At one rank the pair writes the whole gradient, so
 * dxrl_pg_adam_step(gnorm_partial) replaces dxrl_pg_optimizer_step's k_sumsq launch; with a
 * gradient all-reduce in between, the partials are stale and the caller uses the latter. */
int dxrl_pg_fused_pair_gnorm(int32_t device, const dxrl_pg_fused_args* critic, const dxrl_pg_fused_args* actor,
                             double* gnorm_partial, int32_t gnorm_capacity, int32_t* gnorm_blocks, void* stream);
int dxrl_pg_gnorm_blocks(int32_t* blocks);

/* ------------------------------------------------------------------------
 * Evaluation episode programs:
 *   evaluation/evaluator.py:71-271      Evaluator.evaluate_episode / evaluate_heldout_set
 *   evaluation/robustness_tests.py:240-407 RobustnessTester.evaluate_with_noise / run_robustness_sweep
 * A LANE runs a chain of SEGMENTS back to back; a segment is one fresh env
 * instance (DexterousManipulationEnv(curriculum_config=row), so its first reset
 * draws the spawn position and later resets keep the object where it is,
 * manipulation_env.py:156-161), optionally wrapped in CombinedNoiseWrapper(obs
 * std, dyn std) (robustness_tests.py:140-211), running `num_episodes`
 * consecutive reset(seed) -> loop{select_action, step} episodes, each stopping
 * at terminated / truncated / max_steps with success = terminated
 * (evaluator.py:150-158, robustness_tests.py:288-303).  The policy is frozen
 * (evaluator.py:50-70: no update): one of the reference's three, which never
 * read the observation (dxrl_evaluate), or the MLP actor (dxrl_evaluate_mlp);
 * its random stream runs on across the lane's segments, the noise stream
 * restarts with each segment's wrapper.
 *
 * Exact reference order = ONE lane whose segments are the driver's loop (the
 * global np.random stream is consumed serially); the vectorised form = one lane
 * per episode (or per noise level) with its own policy stream.
 * ------------------------------------------------------------------------ */
#define DXRL_EVAL_POLICY_SIMPLE 0    /* frozen SimpleLearner: clip(mean + f32(0 + s g), -1, 1)  (simple_learner.py:59-71) */
#define DXRL_EVAL_POLICY_HEURISTIC 1 /* clip(-0.5f + f32(-0.1 + 0.2 u), -1, 1)         (heuristic_policy.py:38-63) */
#define DXRL_EVAL_POLICY_RANDOM 2    /* Box.sample(): f32(-1 + 2 u)                     (random_policy.py:29-40)    */

typedef struct dxrl_eval_segment {
    int32_t curriculum_row;   /* row of the env's curriculum table                          */
    int32_t num_episodes;     /* consecutive episodes on this instance                      */
    int32_t first_episode;    /* record index of its first episode                           */
    int32_t reserved;
    double obs_noise_std;     /* wrapper observation noise (0 = off; consumes 45 normals per draw) */
    double dyn_noise_std;     /* wrapper dynamics noise (0 = off; 15 normals per step)       */
    int64_t noise_offset;     /* tape mode: first standard normal of this wrapper's stream    */
    int64_t noise_count;      /* tape mode: normals available from noise_offset               */
} dxrl_eval_segment;

typedef struct dxrl_eval_args {
    int32_t num_lanes;               /* <= env num_envs; lane i uses env slot i's weights    */
    int32_t policy;                  /* DXRL_EVAL_POLICY_*                                    */
    int32_t max_steps;               /* episode loop bound (evaluator.py:136)                */
    int32_t total_episodes;          /* record count (bounds check)                          */
    const int32_t* lane_segments;    /* device i32 [num_lanes + 1] CSR offsets into segments */
    const dxrl_eval_segment* segments; /* device                                            */
    const float* mean_action;        /* device f32 [num_lanes][15] (SIMPLE; NULL -> zeros)   */
    double exploration_noise;        /* SIMPLE sigma (simple_learner.py:28)                  */
    /* parity tapes (NULL -> device Philox streams) */
    const double* policy_tape;       /* f64 [num_lanes][policy_stride] raw draws: legacy gauss
                                        (SIMPLE) / next_double (HEURISTIC, RANDOM)           */
    int64_t policy_stride;
    const double* noise_tape;        /* f64 standard normals, addressed by segment offsets   */
    const double* reset_tape;        /* f64 [total_episodes][D+6] resolved reset draws       */
    uint64_t policy_seed, noise_seed, reset_seed; /* Philox keys of the device streams       */
    /* Stream period of dxrl_evaluate_mlp's device Philox streams.  0: the policy stream is keyed by
       the lane index, the noise stream by the segment index, the reset draw by the record index.
       P > 0: by that index modulo P (counters, blocks and stream constants unchanged; records,
       trajectories, policy_used and hist_moments stay addressed by the true index), so indices
       below P keep their keys and lane / segment / record i + m P replays the draws of i: in a
       level-major launch of L levels x P one-episode lanes every level sees the spawns, standard
       normals and action noise of a P-lane launch of that level alone (common random numbers).
       DXRL_E_INVALID: P < 0, P > 0 with any parity tape, P != 0 in dxrl_evaluate.  The field sits
       with the keys it addresses; hist_moments stays the struct's last field. */
    int64_t stream_period;
    /* per-episode records [total_episodes] */
    double* ep_return;               /* episode_reward (f64, sequential sum)                 */
    int32_t* ep_length;              /* episode_steps                                        */
    uint8_t* ep_success;             /* terminated at the last step                          */
    uint8_t* ep_contacts;            /* num_contacts of the last step's info                 */
    uint8_t* contact_hist;           /* u8 [total_episodes][max_steps] per-step num_contacts
                                        (contact_history, evaluator.py:148-150; nullable)   */
    int32_t* policy_used;            /* i32 [num_lanes] policy draws consumed (nullable)     */
    int32_t* status;                 /* i32 [1] device error word: 1 = a tape ran out        */
    /* trajectories (nullable; failure_logger.py:242-297 EpisodeRecorder, evaluator.py:101-152):
       obs_traj f32 [total_episodes][max_steps + 1][45] -- the reset observation, then the
       observation after every step; act_traj f32 [total_episodes][max_steps][15] -- the policy's
       action of every step.  Rows past an episode's length are left untouched. */
    float* obs_traj;
    float* act_traj;
    /* device i32 [1] scratch owned by the caller: this launch's work-queue counter (zeroed on
       the stream by the call).  Required by the default (work-queue) kernel; give each launch
       that may run concurrently with another its own counter. */
    int32_t* work_queue;
    /* i32 [total_episodes][5] (nullable): S1 = sum c, S2 = sum c^2, first-five sum, last-five sum
       and peak of the episode's per-step num_contacts c, accumulated inside the step loop and
       written once with the episode's other records -- what dxrl_failure_summarize needs of the
       history, so contact_hist may then be NULL and nothing per step reaches memory for it.
       Needs max_steps <= 4096 (the packed accumulators), else DXRL_E_INVALID. */
    int32_t* hist_moments;
} dxrl_eval_args;

int dxrl_evaluate(dxrl_env* env, const dxrl_eval_args* args, void* stream);

/* The same episode programs with the frozen MLP actor of the policy-gradient learner as the
 * policy (no reference counterpart for the network; the loops are
 * evaluator.py:71-181 / robustness_tests.py:240-310 as above).  At every step the action is
 *   deterministic (action_std NULL):  a = clip(mu(obs), -1, 1), no policy draw, policy_used 0;
 *   stochastic:                       a = clip(mu(obs) + nz, -1, 1) with, per action dim k,
 *     tape mode    nz_k = f32(0 + (double)action_std[k] g_k), 15 raw normals of the lane's
 *                  policy_tape per step;
 *     device mode  nz_k = action_std[k] z_k from the lane's Philox policy stream (Box-Muller,
 *                  addressed like DXRL_EVAL_POLICY_SIMPLE's),
 * where mu = tanh(tanh(x W1^T) W2^T + b2) W3^T + b3 on bf16 MFMA tiles exactly as dxrl_pg_rollout
 * computes it (the 16 env rows of a workgroup are one M = 16 tile; weights from `packed`, b2 / b3
 * from `params`) and x is the bf16-rounded observation the loop hands its policy: the env's 45
 * elements, inside a noisy segment plus the wrapper's observation noise f32(0 + std g)
 * (robustness_tests.py:199-207) -- in tape mode the 45 normals per observation at the cursor
 * positions dxrl_evaluate only skips, in device mode the segment's Philox noise stream.  The
 * kernel evaluates no exp: the caller passes exp(log_std).  obs_traj holds the observation the
 * policy saw (noisy when the segment is), act_traj the policy's clipped action.
 * args keeps dxrl_evaluate's layout: args->policy must be DXRL_EVAL_POLICY_MLP, mean_action and
 * exploration_noise are ignored, work_queue is required, and a policy_tape in deterministic mode
 * is an error.  dxrl_evaluate itself does not accept DXRL_EVAL_POLICY_MLP. */
#define DXRL_EVAL_POLICY_MLP 3
typedef struct dxrl_eval_mlp {
    const void*  packed;      /* bf16 pack of dxrl_pg_pack_weights (16-byte aligned)            */
    const float* params;      /* f32 master (layer-2 / head biases)                              */
    const float* action_std;  /* f32 [15]; NULL = deterministic (no policy draws)                */
} dxrl_eval_mlp;
int dxrl_evaluate_mlp(dxrl_env* env, const dxrl_eval_args* args, const dxrl_eval_mlp* mlp, void* stream);

/* ------------------------------------------------------------------------
 * Episode summaries on the device: evaluation/metrics.py:39-103,128-206
 * (EvaluationMetrics.classify_failure in rule order and the sums behind
 * compute_aggregate_metrics), over the record buffers dxrl_evaluate /
 * dxrl_evaluate_mlp wrote on the same stream.  Two launches, stream-ordered
 * behind the episode kernel, no host synchronisation: a per-episode pass (all
 * the contact_hist traffic; failure code and history moments of every episode)
 * and a per-group pass over a CSR group table.  An episode may belong to several
 * groups or to none ("per object", "per seed" and "overall" are three sets of
 * groups of one table).
 *
 * ep_code: -1 = success, else the index into the FailureType enumeration in its
 * declaration order (0 slippage, 1 unstable_contacts, 2 misaligned_grasp,
 * 3 timeout, 4 object_dropped, 5 insufficient_contacts); rules in the order
 * TIMEOUT, OBJECT_DROPPED, UNSTABLE_CONTACTS (n > 5), SLIPPAGE (n > 10),
 * MISALIGNED_GRASP, INSUFFICIENT_CONTACTS.  np.var(counts) > 2.0 is decided
 * exactly in integers, n S2 - S1^2 > 2 n^2; the slippage rule is the f64
 * expression (L / 5.0) - (F / 5.0) < -1.0.
 * TIE ROWS: an episode still open at the variance rule with n > 5 and
 * n S2 - S1^2 == 2 n^2.  np.var's own rounding decides those, so the kernel
 * classifies them as not unstable, lists them in tie_list (ascending) and
 * counts them in slot 13 of every group that holds them; the caller settles them
 * with np.var on those rows' histories and moves one failure-code count per
 * holding group where np.var says unstable.
 *
 * group_stats i64 [G][16]: 0 episodes, 1 successes, 2 sum steps, 3 sum steps^2,
 * 4 sum contacts, 5 sum steps over successes, 6 sum contacts over successes,
 * 7..12 episodes per failure code 0..5, 13 tie rows, 14-15 zero.
 * group_return f64 [G][3]: count, mean, M2 (sum of squared deviations) of
 * ep_return, accumulated about the group's first member's return and merged
 * with Chan et al.'s update in a fixed order: bit-identical from run to run (no
 * floating-point atomics), and no cancellation for returns of the form
 * big + small.
 * status i32 [1] (zeroed on the stream by the call): bit 0 = a group offset or a
 * member episode index was out of range (that group / member is skipped, nothing
 * is written out of bounds); bit 1 = more tie rows than tie_cap (tie_count still
 * holds the true count).
 * ------------------------------------------------------------------------ */
#define DXRL_SUMMARY_MAX_STEPS 4096 /* larger max_steps -> DXRL_E_INVALID */
typedef struct dxrl_eval_summary_args {
    int32_t total_episodes;          /* E                                                    */
    int32_t max_steps;               /* contact_hist row pitch and the TIMEOUT bound         */
    int32_t success_threshold;       /* MISALIGNED_GRASP: 0 < num_contacts < threshold       */
    int32_t num_groups;              /* G                                                    */
    int32_t num_members;             /* entries of group_episodes (bounds check)             */
    int32_t tie_cap;                 /* entries of tie_list                                  */
    /* device inputs: the episode kernel's records */
    const int32_t* ep_length;        /* i32 [E]                                              */
    const uint8_t* ep_success;       /* u8  [E]                                              */
    const uint8_t* ep_contacts;      /* u8  [E] num_contacts == final_contacts               */
    const double*  ep_return;        /* f64 [E]                                              */
    const uint8_t* contact_hist;     /* u8  [E][max_steps]; rows need not be 4-byte aligned  */
    const int32_t* group_offsets;    /* i32 [G + 1] CSR offsets into group_episodes          */
    const int32_t* group_episodes;   /* i32 [num_members] episode indices                    */
    /* device outputs */
    uint8_t* ep_work;                /* u8  [E] scratch between the two launches (required)  */
    int8_t*  ep_code;                /* i8  [E]    (nullable)                                */
    int32_t* ep_moments;             /* i32 [E][4] S1, S2, first-five sum, last-five sum (nullable) */
    int64_t* group_stats;            /* i64 [G][16]                                          */
    double*  group_return;           /* f64 [G][3]                                           */
    int32_t* tie_count;              /* i32 [1]                                              */
    int32_t* tie_list;               /* i32 [tie_cap]                                        */
    int32_t* status;                 /* i32 [1]                                              */
} dxrl_eval_summary_args;

int dxrl_eval_summarize(int32_t device, const dxrl_eval_summary_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Failure-mode study on the device: the taxonomy of
 * evaluation/failure_taxonomy.py:156-239 (FailureClassifier.classify: mode and
 * confidence of every episode) and, per group and failure mode, the sums
 * behind evaluation/failure_statistics.py:34-159 (compute_failure_distribution,
 * compute_correlations) and evaluation/failure_analysis.py:61-99
 * (analyze_failure_modes), over the record buffers of dxrl_evaluate /
 * dxrl_evaluate_mlp.  Two launches, stream-ordered behind the episode kernel, no
 * host synchronisation; the group table has dxrl_eval_summarize's semantics.
 *
 * The history of an episode enters either as its contact_hist row or as the five
 * words the episode kernels accumulate (dxrl_eval_args.hist_moments: S1, S2,
 * first-five sum F, last-five sum L, peak); exactly one of the two is given.
 * n = ep_length clamped to [0, max_steps], num = n S2 - S1^2, nc = ep_contacts
 * (num_contacts == final_contacts in these records; peak = nc when n == 0).
 * ep_mode: -1 = success, else the index into list(FailureMode) (0 slippage,
 * 1 unstable_grasp, 2 misalignment, 3 timeout, 4 object_dropped,
 * 5 insufficient_contacts), by the rules in this order:
 *   1 ep_length >= timeout_steps                       timeout        1.0
 *   2 nc == 0 and peak > 0                             object_dropped 1.0
 *   3 n > 10, trend = L / 5.0 - F / 5.0 < -1.0 (f64),
 *     peak >= 1                                        slippage       min(1, |trend| / 2)
 *   4 n > 5, num > 2 n^2                               unstable_grasp min(1, var / 5),
 *                                                      var = (double)num / (double)(n n)
 *   5 1 <= nc <= 2 and (n <= 1 or num < n^2)           misalignment   0.8
 *   6 peak < success_threshold                         insufficient_contacts 1.0
 *   7 otherwise                                        insufficient_contacts 0.5
 * timeout_steps is classify's max_steps argument, not the history pitch: a study
 * may classify at a larger bound than its episode loop ran to.
 * TIE ROWS: an episode that reaches rule 4 with n > 5 and num == 2 n^2, or rule 5
 * with 1 <= nc <= 2, n > 1 and num == n^2; np.var's own rounding decides those.
 * ep_mode / ep_confidence hold the exact comparison's answer (not unstable, not
 * misaligned).  With contact_hist the tie rows are left out of mode_stats and
 * mode_props (the caller classifies those rows and merges them); with
 * hist_moments there is no row to settle with and they are included as decided.
 * In both forms they are listed ascending in tie_list and counted per group.
 *
 * mode_stats i64 [G][6][8]: 0 episodes, 1 sum steps, 2 sum steps^2, 3 sum final
 * contacts, 4 sum final contacts^2, 5-7 zero.
 * group_totals i64 [G][4]: 0 episodes, 1 successes, 2 tie rows, 3 zero.
 * mode_props f64 [G][6][3][5]: count, mean, M2, min, max of object size, mass and
 * friction (ep_props columns), accumulated about the first member of the (group,
 * mode) and merged with Chan et al.'s update in a fixed tree (no floating-point
 * atomics: bit-identical from run to run); min and max are exact.  All zero for an
 * empty (group, mode).
 * status: as dxrl_eval_summarize (bit 0 group table out of range, bit 1 more tie
 * rows than tie_cap; tie_count holds the true count).
 * ------------------------------------------------------------------------ */
#define DXRL_FAILURE_MODES 6
typedef struct dxrl_failure_summary_args {
    int32_t total_episodes;          /* E                                                    */
    int32_t max_steps;               /* contact_hist row pitch (<= DXRL_SUMMARY_MAX_STEPS)   */
    int32_t timeout_steps;           /* the timeout bound of rule 1                          */
    int32_t success_threshold;       /* rule 6                                               */
    int32_t num_groups;              /* G                                                    */
    int32_t num_members;             /* entries of group_episodes (bounds check)             */
    int32_t tie_cap;                 /* entries of tie_list                                  */
    int32_t reserved;
    /* device inputs */
    const int32_t* ep_length;        /* i32 [E]                                              */
    const uint8_t* ep_success;       /* u8  [E]                                              */
    const uint8_t* ep_contacts;      /* u8  [E]                                              */
    const double*  ep_props;         /* f64 [E][3] object size, mass, friction               */
    const uint8_t* contact_hist;     /* u8  [E][max_steps], or NULL                          */
    const int32_t* hist_moments;     /* i32 [E][5] S1, S2, F, L, peak, or NULL               */
    const int32_t* group_offsets;    /* i32 [G + 1]                                          */
    const int32_t* group_episodes;   /* i32 [num_members]                                    */
    /* device outputs */
    uint8_t* ep_work;                /* u8  [E] scratch between the two launches (required)  */
    int8_t*  ep_mode;                /* i8  [E]  (nullable)                                  */
    double*  ep_confidence;          /* f64 [E]  (nullable; 0 for a success)                 */
    int64_t* mode_stats;             /* i64 [G][6][8]                                        */
    int64_t* group_totals;           /* i64 [G][4]                                           */
    double*  mode_props;             /* f64 [G][6][3][5]                                     */
    int32_t* tie_count;              /* i32 [1]                                              */
    int32_t* tie_list;               /* i32 [tie_cap]                                        */
    int32_t* status;                 /* i32 [1]                                              */
} dxrl_failure_summary_args;

int dxrl_failure_summarize(int32_t device, const dxrl_failure_summary_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Robustness study on the device: evaluation/robustness_analysis.py:12-77
 * (analyze_robustness_results: the degradation of every noise level against its
 * baseline) on top of the episode rules and group sums of
 * evaluation/metrics.py:39-103,128-206, over the record buffers of dxrl_evaluate /
 * dxrl_evaluate_mlp.  Two launches, stream-ordered behind the episode kernel, no
 * host synchronisation: a per-group pass that classifies its members inline, and
 * a per-group degradation pass behind it.  The group table has
 * dxrl_eval_summarize's semantics.
 *
 * The history of an episode enters only as the five words the episode kernels
 * accumulate (dxrl_eval_args.hist_moments: S1, S2, first-five sum F, last-five
 * sum L, peak; the peak is not read): there is no contact_hist argument.  ep_code
 * and the rules are dxrl_eval_summarize's, applied to (ep_length, ep_success,
 * ep_contacts, S1, S2, F, L), np.var(counts) > 2.0 again decided as
 * n S2 - S1^2 > 2 n^2.
 * TIE ROWS (n > 5 and n S2 - S1^2 == 2 n^2 at the variance rule) are classified
 * as not unstable, counted in slot 13 and listed ascending in tie_list, and they
 * stay so decided: without a history row the caller cannot ask np.var (the stance
 * of dxrl_failure_summarize's hist_moments form).
 *
 * group_stats i64 [G][16] and group_return f64 [G][3]: dxrl_eval_summarize's
 * tables, same member-to-thread assignment, accumulation and merge order --
 * bit-identical to it on the same records (tie rows before its caller's fix-up).
 * level_table f64 [G][4], b = baseline_group[g], each column formed with exactly
 * these f64 operations in this order (the reference's Python floats, bit for bit):
 *   0 success_rate           = successes / episodes
 *   1 mean_episode_length    = sum steps / episodes
 *   2 degradation            = success_rate[b] - success_rate[g]
 *   3 degradation_percentage = success_rate[b] > 0
 *                                ? degradation / success_rate[b] * 100 : 0.0
 * Columns 0-1 are NaN for an empty group; columns 2-3 are NaN when b == -1 (no
 * baseline) or when either group is empty.  b may equal g or exceed it.
 * status: bits 0 and 1 as dxrl_eval_summarize; bit 2 = a baseline_group entry
 * outside [-1, G) (that row's columns 2-3 are NaN, nothing is read out of bounds).
 * ------------------------------------------------------------------------ */
typedef struct dxrl_robustness_summary_args {
    int32_t total_episodes;          /* E                                                    */
    int32_t max_steps;               /* the TIMEOUT bound (1..DXRL_SUMMARY_MAX_STEPS)        */
    int32_t success_threshold;       /* MISALIGNED_GRASP: 0 < num_contacts < threshold       */
    int32_t num_groups;              /* G                                                    */
    int32_t num_members;             /* entries of group_episodes (bounds check)             */
    int32_t tie_cap;                 /* entries of tie_list                                  */
    /* device inputs: the episode kernel's records */
    const int32_t* ep_length;        /* i32 [E]                                              */
    const uint8_t* ep_success;       /* u8  [E]                                              */
    const uint8_t* ep_contacts;      /* u8  [E] num_contacts == final_contacts               */
    const double*  ep_return;        /* f64 [E]                                              */
    const int32_t* hist_moments;     /* i32 [E][5] S1, S2, F, L, peak                        */
    const int32_t* group_offsets;    /* i32 [G + 1] CSR offsets into group_episodes          */
    const int32_t* group_episodes;   /* i32 [num_members] episode indices                    */
    const int32_t* baseline_group;   /* i32 [G] group each level is compared with, -1 = none */
    /* device outputs */
    int64_t* group_stats;            /* i64 [G][16]                                          */
    double*  group_return;           /* f64 [G][3]                                           */
    double*  level_table;            /* f64 [G][4]                                           */
    int8_t*  ep_code;                /* i8  [E]    (nullable)                                */
    int32_t* tie_count;              /* i32 [1]                                              */
    int32_t* tie_list;               /* i32 [tie_cap]                                        */
    int32_t* status;                 /* i32 [1]                                              */
} dxrl_robustness_summary_args;

int dxrl_robustness_summarize(int32_t device, const dxrl_robustness_summary_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Training-run summaries on the device: evaluation/curriculum_ablation.py:137-203,
 * 269-282 (compute_convergence_metrics, aggregate_metrics) and
 * evaluation/component_ablation.py:168-186,285-322 (the window-20 convergence step,
 * the final success rate, compute_ablation_statistics), over the episode records
 * dxrl_rollout_simple / dxrl_rollout_curriculum wrote on the same stream.  Up to two
 * launches, stream-ordered behind the rollout, no host synchronisation: a LANE PASS
 * (a wavefront per lane = per training run) that writes rows lane_offset ..
 * lane_offset + num_lanes of a study-wide lane table, and a GROUP PASS over the whole
 * lane table with a CSR group table (dxrl_eval_summarize's semantics: a lane may be in
 * several groups or in none).  A study whose runs lie in several record buffers (a
 * dense and a sparse env handle) calls once per buffer; the group pass runs in the
 * calls that give group_stats (the last one), the lane pass in those with num_lanes > 0.
 *
 * Lane pass, E = lane_episodes[lane] (ep_count of a one-launch study), w = window,
 * r / steps / success = the lane's first E records:
 * lane_ints i64 [total_lanes][8]:
 *   0 episodes E                  1 sum of steps          2 successes
 *   3 final_window_successes: successes among the last min(w, E) episodes
 *   4 convergence_step: the first i in [w, E) with popcount(success[i-w : i]) >=
 *     min_count, else -1 (np.mean(window) >= 0.5 decided in integers when min_count is
 *     the smallest c with c / w >= 0.5)
 *   5 reward_convergence_episode: the first i with ma_i >= reward_threshold, reported as
 *     i + w - 1, else -1.  E >= w: ma_i = sum over j < w, left to right in f64, of
 *     r[i+j] * (1.0 / w), i in [0, E - w].  E < w: ma_i = r[i] (an exact comparison).
 *   6 final_level: ep_level[E - 1], -1 without ep_level
 *   7 flags: bit 0 tie lane, bit 1 skipped lane (every other column 0 / -1)
 * lane_reals f64 [total_lanes][4]: 0 count, 1 mean, 2 M2 of the returns (accumulated
 *   about r[0]: episode e on wave lane e % 64 in ascending order, Welford; then Chan et
 *   al.'s merge over the 64 partials in a fixed tree), 3 final_reward = the left-to-right
 *   sum of the last min(w, E) returns, divided by their number.
 * TIE LANES (E >= w only): np.convolve does not sum in this order, so a crossing that
 * lies within rounding is not decided here.  A lane is a tie lane if some i at or before
 * its first crossing (any i if it has none) has
 *   |ma_i - reward_threshold| <= 64 eps w max_j |r[i+j] * (1.0 / w)|,  eps = 2^-52.
 * Column 5 then holds the left-to-right answer; tie lanes are listed ascending (lane
 * table rows) in tie_list, counted in tie_count and in slot 14 of every group holding
 * them; the caller settles them with compute_convergence_metrics on those lanes'
 * returns and adjusts the group sums.
 *
 * Group pass (skipped lanes are left out):
 * group_stats i64 [G][16]: 0 lanes, 1 sum E, 2 sum steps_l, 3 sum steps_l^2 (steps_l =
 *   column 1), 4 sum / 5 sum of squares / 6 min / 7 max of final_window_successes,
 *   8 converged lanes, 9 sum / 10 sum of squares of convergence_step, 11 reward-converged
 *   lanes, 12 sum / 13 sum of squares of reward_convergence_episode, 14 tie lanes,
 *   15 sum of successes.
 * group_metrics f64 [G][5][3]: count, mean, M2 over the group's lanes of 0 reward
 *   variance (M2 / count), 1 reward std (sqrt of it), 2 coefficient of variation (std /
 *   mean), 3 final_reward, 4 mean reward; accumulated about the group's first member's
 *   value and merged with Chan et al.'s update in a fixed tree (no floating-point
 *   atomics: bit-identical from run to run).  A lane whose mean reward is exactly 0 has
 *   an infinite CV: it is left out of metric 2, so lanes - count[2] such lanes exist.
 * status i32 [1] (zeroed on the stream by the call): bit 0 = a group offset or a member
 * lane was out of range (skipped, nothing is accessed out of bounds); bit 1 = more tie
 * lanes than tie_cap (tie_count holds the true count); bit 2 = a lane had E <= 0 or
 * E > record_cap (skipped); bit 3 = the lanes of a group do not share one E (its integer
 * rate and length sums are then not the reference's statistics: use the lane table).
 * window outside 1..64, record_cap <= 0, rows outside the lane table or a null required
 * pointer: DXRL_E_INVALID before any launch.
 * ------------------------------------------------------------------------ */
#define DXRL_STUDY_LANE_INTS 8
#define DXRL_STUDY_LANE_REALS 4
#define DXRL_STUDY_METRICS 5
typedef struct dxrl_study_summary_args {
    int32_t num_lanes;               /* N: lanes of this record buffer (0 = no lane pass)    */
    int32_t record_cap;              /* row pitch of the record buffers                      */
    int32_t lane_offset;             /* first lane-table row this call writes                */
    int32_t total_lanes;             /* rows of the lane table                               */
    int32_t window;                  /* w, 1..64                                             */
    int32_t min_count;               /* successes in a window that count as converged        */
    int32_t num_groups;              /* G                                                    */
    int32_t num_members;             /* entries of group_lanes (bounds check)                */
    int32_t tie_cap;                 /* entries of tie_list                                  */
    int32_t reserved;
    double reward_threshold;
    /* device inputs */
    const double*  ep_return;        /* f64 [N][record_cap]                                  */
    const int32_t* ep_length;        /* i32 [N][record_cap]                                  */
    const uint8_t* ep_success;       /* u8  [N][record_cap]                                  */
    const int32_t* ep_level;         /* i32 [N][record_cap] (nullable)                       */
    const int32_t* lane_episodes;    /* i32 [N] E of every lane                              */
    const int32_t* group_offsets;    /* i32 [G + 1] CSR offsets into group_lanes             */
    const int32_t* group_lanes;      /* i32 [num_members] lane-table rows                    */
    /* device outputs */
    int64_t* lane_ints;              /* i64 [total_lanes][8]                                 */
    double*  lane_reals;             /* f64 [total_lanes][4]                                 */
    int64_t* group_stats;            /* i64 [G][16]; NULL = no group pass in this call       */
    double*  group_metrics;          /* f64 [G][5][3]                                        */
    int32_t* tie_count;              /* i32 [1]                                              */
    int32_t* tie_list;               /* i32 [tie_cap]                                        */
    int32_t* status;                 /* i32 [1]                                              */
} dxrl_study_summary_args;

int dxrl_study_summarize(int32_t device, const dxrl_study_summary_args* args, void* stream);

/* ---------------------------------------------------------------------------
 * Per-iteration training log (csrc/dxrl_pg_log.hip).  One call per policy-gradient
 * iteration, enqueued behind the optimiser step: it reads what the iteration left on the
 * device and writes row `row` of the f64 table log[cap][DXRL_PG_LOG_COLS]; nothing returns
 * to the host.  Samples are time-major, m = t * num_envs + i, M = num_envs * horizon.
 *
 * Columns (enum dxrl_pg_log_col):
 *   iteration, env_steps       the host scalars
 *   episodes                   sum of ep_count
 *   mean_return, mean_length,  sums of ep_sum_return / ep_sum_length / ep_successes over
 *   success_rate               episodes (NaN when episodes == 0)
 *   mean_step_reward           mean of rew
 *   done_fraction              mean of done (count of non-zero bytes / M)
 *   value_mean                 mean of values[m], m < M (the bootstrap slot values[M ..] is
 *                              never read)
 *   target_mean, target_var    population mean and variance of ret
 *   residual_var               population variance of (double)ret[m] - (double)values[m]
 *   explained_variance         1 - residual_var / target_var (NaN when target_var == 0)
 *   adv_mean, adv_std          stats[2], stats[4] (dxrl_pg_gae / dxrl_pg_adv_combine)
 *   policy_loss, value_mse,    the four columns of loss_partial summed over loss_blocks,
 *   clip_frac, approx_kl       divided by loss_rows
 *   grad_norm                  sqrt(gnorm2[0])
 *   is_best, window_mean       below
 * Columns from DXRL_PG_LOG_NAMED up to DXRL_PG_LOG_COLS are written as 0.
 *
 * Sums are f64; variances come from (count, mean, M2) triples merged with Chan's update in
 * a fixed order (workgroup partials in `partial`, then one finishing workgroup): no
 * floating-point atomics, and the same inputs give the same bytes on every call.
 *
 * Header (dxrl_pg_log_header, device memory, initialised by the caller to rows_written 0,
 * best_row -1, converged_row -1, best_score -inf):
 *   keep-best (score_col >= 0): is_best = 1 iff episodes >= min_episodes and
 *     log[row][score_col] > best_score (strict: the first maximum wins, a NaN is never best);
 *     best_score / best_row are then updated, and a second launch copies params to
 *     best_params (num_params f32) iff is_best -- the flag is read on the device.
 *   convergence (conv_col >= 0): window_mean = mean of log[row - W + 1 .. row][conv_col],
 *     summed oldest first (NaN while row < W - 1); converged_row = the first row whose
 *     window_mean > conv_threshold (strict; a NaN in the window does not converge).
 *   rows_written = row + 1.
 * score_col / conv_col must be < DXRL_PG_LOG_IS_BEST (or < 0: off; is_best 0 / window_mean
 * NaN).  DXRL_E_INVALID before any launch: null args or required pointer, num_envs or
 * horizon < 1, row outside [0, cap), a column index out of range, conv_col >= 0 with
 * conv_window < 1, loss_blocks < 0, loss_rows < 1, partial_doubles smaller than
 * dxrl_pg_log_partial_doubles(num_envs, horizon), score_col >= 0 with params but no
 * best_params (both null: no copy).
 * ------------------------------------------------------------------------ */
#define DXRL_PG_LOG_COLS 24
enum dxrl_pg_log_col {
    DXRL_PG_LOG_ITERATION = 0,
    DXRL_PG_LOG_ENV_STEPS,
    DXRL_PG_LOG_EPISODES,
    DXRL_PG_LOG_MEAN_RETURN,
    DXRL_PG_LOG_MEAN_LENGTH,
    DXRL_PG_LOG_SUCCESS_RATE,
    DXRL_PG_LOG_MEAN_STEP_REWARD,
    DXRL_PG_LOG_DONE_FRACTION,
    DXRL_PG_LOG_VALUE_MEAN,
    DXRL_PG_LOG_TARGET_MEAN,
    DXRL_PG_LOG_TARGET_VAR,
    DXRL_PG_LOG_RESIDUAL_VAR,
    DXRL_PG_LOG_EXPLAINED_VARIANCE,
    DXRL_PG_LOG_ADV_MEAN,
    DXRL_PG_LOG_ADV_STD,
    DXRL_PG_LOG_POLICY_LOSS,
    DXRL_PG_LOG_VALUE_MSE,
    DXRL_PG_LOG_CLIP_FRAC,
    DXRL_PG_LOG_APPROX_KL,
    DXRL_PG_LOG_GRAD_NORM,
    DXRL_PG_LOG_IS_BEST,
    DXRL_PG_LOG_WINDOW_MEAN,
    DXRL_PG_LOG_NAMED /* 22 named columns, padded to DXRL_PG_LOG_COLS (a multiple of 4) */
};

typedef struct dxrl_pg_log_header {
    int64_t rows_written;
    int64_t best_row;      /* -1: none yet */
    int64_t converged_row; /* -1: not converged */
    int64_t reserved;
    double best_score;     /* -inf: none yet */
    double reserved_f64[3];
} dxrl_pg_log_header;

typedef struct dxrl_pg_log_args {
    int64_t num_envs;                /* N                                                    */
    int64_t horizon;                 /* T                                                    */
    int64_t row;                     /* table row this call writes, 0 <= row < cap           */
    int64_t cap;                     /* rows of the table                                    */
    int64_t iteration;               /* column 0                                             */
    int64_t env_steps;               /* column 1 (cumulative)                                */
    int64_t loss_blocks;             /* rows of loss_partial                                 */
    int64_t loss_rows;               /* samples of the last train pass                       */
    int64_t min_episodes;            /* keep-best gate                                       */
    int64_t num_params;              /* f32 elements of params / best_params                 */
    int64_t partial_doubles;         /* f64 elements of partial                              */
    int32_t score_col;               /* keep-best column, < 0: off                           */
    int32_t conv_col;                /* convergence column, < 0: off                         */
    int32_t conv_window;             /* W >= 1                                               */
    int32_t reserved;
    double conv_threshold;
    /* device inputs */
    const int32_t* ep_count;         /* i32 [N]                                              */
    const double*  ep_sum_return;    /* f64 [N]                                              */
    const int32_t* ep_sum_length;    /* i32 [N]                                              */
    const int32_t* ep_successes;     /* i32 [N]                                              */
    const float*   rew;              /* f32 [M]                                              */
    const float*   ret;              /* f32 [M]                                              */
    const uint8_t* done;             /* u8  [M]                                              */
    const float*   values;           /* f32 [(T + 1) N]; only [0, M) is read                 */
    const double*  stats;            /* f64 [8] (dxrl_pg_gae)                                */
    const double*  loss_partial;     /* f64 [loss_blocks][4]                                 */
    const double*  gnorm2;           /* f64 [1]                                              */
    const float*   params;           /* f32 [num_params] (nullable with best_params)         */
    /* device scratch and outputs */
    double* partial;                 /* f64 [partial_doubles] scratch                        */
    float*  best_params;             /* f32 [num_params] (nullable with params)              */
    double* log;                     /* f64 [cap][DXRL_PG_LOG_COLS]                          */
    dxrl_pg_log_header* header;
} dxrl_pg_log_args;

/* f64 elements of dxrl_pg_log_row's `partial` scratch for num_envs x horizon samples. */
int dxrl_pg_log_partial_doubles(int64_t num_envs, int64_t horizon, int64_t* out);
int dxrl_pg_log_row(int32_t device, const dxrl_pg_log_args* args, void* stream);

/* ---------------------------------------------------------------------------
 * The training log of a sharded trainer (csrc/dxrl_pg_log.hip): dxrl_pg_log_row split where the
 * ranks must meet.  Per logged iteration every rank calls dxrl_pg_log_rank_pack on its own tape,
 * all-gathers the records in rank order (the caller's collective, on the same stream) and calls
 * dxrl_pg_log_row_world on the gathered records; since every rank finishes from the same bytes,
 * table, header and best_params are identical on all ranks.
 *
 * dxrl_pg_log_rank_pack reduces the rank's num_envs x horizon samples, episode counters and
 * loss_partial blocks into record[DXRL_PG_LOG_RANK_DOUBLES] (enum dxrl_pg_log_rank_col), in the
 * reduction order of dxrl_pg_log_row.  It writes neither log nor header nor best_params.
 *   samples                    the rank's sample count, num_envs * horizon
 *   reward_sum, value_sum      sums of rew and of values[m], m < M
 *   done_count                 non-zero done bytes
 *   target_mean, target_m2     mean and sum of squared deviations of ret (count: samples)
 *   residual_mean, residual_m2 the same of (double)ret[m] - (double)values[m]
 *   episodes, length_sum,      sums of ep_count / ep_sum_length / ep_successes / ep_sum_return
 *   successes, return_sum
 *   policy_loss_sum, value_se_sum, clip_sum, kl_sum
 *                              the four columns of loss_partial summed over loss_blocks
 *   loss_rows                  args->loss_rows
 * Entries from DXRL_PG_LOG_RANK_NAMED up to DXRL_PG_LOG_RANK_DOUBLES are written as 0.
 *
 * dxrl_pg_log_row_world merges records[world][DXRL_PG_LOG_RANK_DOUBLES] in rank order (sums: f64
 * additions; the two triples: Chan's update) and writes row `row` as dxrl_pg_log_row does, with
 * every per-sample column over the sum of the records' samples and the loss columns over the sum
 * of their loss_rows -- shards need not be equal.  adv_mean, adv_std and grad_norm come from
 * stats and gnorm2 (global already on a sharded trainer); iteration and env_steps from args
 * (env_steps: the caller's global count).  Keep-best, convergence, the header and the conditional
 * copy of params are dxrl_pg_log_row's.  rank_log (nullable): f64 [cap][world]
 * [DXRL_PG_LOG_RANK_DOUBLES]; row `row` receives the gathered records.  With world == 1, pack
 * followed by row_world writes the bytes dxrl_pg_log_row writes.  The sample inputs of args are
 * not read by row_world but are checked as dxrl_pg_log_row checks them.
 * DXRL_E_INVALID before any launch: null record / records, world < 1, and everything
 * dxrl_pg_log_row refuses.
 * ------------------------------------------------------------------------ */
#define DXRL_PG_LOG_RANK_DOUBLES 20
enum dxrl_pg_log_rank_col {
    DXRL_PG_LOG_RANK_SAMPLES = 0,
    DXRL_PG_LOG_RANK_REWARD_SUM,
    DXRL_PG_LOG_RANK_VALUE_SUM,
    DXRL_PG_LOG_RANK_DONE_COUNT,
    DXRL_PG_LOG_RANK_TARGET_MEAN,
    DXRL_PG_LOG_RANK_TARGET_M2,
    DXRL_PG_LOG_RANK_RESIDUAL_MEAN,
    DXRL_PG_LOG_RANK_RESIDUAL_M2,
    DXRL_PG_LOG_RANK_EPISODES,
    DXRL_PG_LOG_RANK_LENGTH_SUM,
    DXRL_PG_LOG_RANK_SUCCESSES,
    DXRL_PG_LOG_RANK_RETURN_SUM,
    DXRL_PG_LOG_RANK_POLICY_LOSS_SUM,
    DXRL_PG_LOG_RANK_VALUE_SE_SUM,
    DXRL_PG_LOG_RANK_CLIP_SUM,
    DXRL_PG_LOG_RANK_KL_SUM,
    DXRL_PG_LOG_RANK_LOSS_ROWS,
    DXRL_PG_LOG_RANK_NAMED /* 17 named entries, padded to DXRL_PG_LOG_RANK_DOUBLES (160 bytes) */
};

int dxrl_pg_log_rank_pack(int32_t device, const dxrl_pg_log_args* args, double* record, void* stream);
int dxrl_pg_log_row_world(int32_t device, const dxrl_pg_log_args* args, const double* records, int32_t world,
                          double* rank_log, void* stream);

/* ---------------------------------------------------------------------------
 * Held-out validation row of a training run (csrc/dxrl_pg_val.hip).  One call per validation,
 * enqueued behind dxrl_evaluate_mlp on the same stream: it reduces the episode records of an
 * object-major evaluation (G objects x K episodes, E = G K, the record of object o, episode k
 * at o K + k -- Evaluator.heldout_program's layout) into row `row` of the f64 table
 * val[cap][DXRL_PG_VAL_COLS]; nothing returns to the host.
 *
 * Columns (enum dxrl_pg_val_col):
 *   iteration, env_steps,      the host scalars; train_row is the row of the training log this
 *   train_row                  validation follows
 *   episodes                   E
 *   successes, success_rate    count of non-zero ep_success bytes, and that count / E
 *   mean_return, return_std    population mean and standard deviation of ep_return
 *                              (np.mean / np.std, EvalSummary.std_reward's definition)
 *   mean_length                mean of ep_length
 *   mean_success_length        mean of ep_length over the successes (NaN with none)
 *   mean_contacts              mean of ep_contacts
 *   min_object_success_rate    min over objects of successes(o) / K
 *   objects_solved             objects with (double)successes(o) / K >= solve_threshold
 *   eval_status                the episode kernel's status word
 *   is_best, since_best        below
 *
 * Integer sums are exact; the return moments are (count, mean, M2) triples of ep_return - ep_return[0]
 * (the shift is exact for returns of one magnitude, so a large common offset does not cancel)
 * merged with Chan's update in a fixed order: records in index order inside a thread, lanes by
 * shuffles, waves and workgroup partials in index order.  No floating-point atomics; the same
 * inputs give the same bytes on every call.
 *
 * Header (dxrl_pg_val_header, device memory, initialised by the caller to rows_written 0,
 * best_row -1, stopped_row -1, since_best 0, best_score -inf):
 *   keep-best (score_col >= 0): is_best = 1 iff eval_status == 0 and
 *     val[row][score_col] > best_score + min_delta (strict: the first maximum wins, a NaN is
 *     never best, and with best_score == -inf any finite score is); best_score / best_row are
 *     then updated, and a following launch copies params to best_params (num_params f32) iff
 *     is_best -- the flag is read on the device.
 *   patience: since_best = 0 if is_best, else the header's since_best (the previous row's) + 1;
 *     with patience > 0, stopped_row = the first row with since_best >= patience, never
 *     overwritten once set.
 *   rows_written = row + 1.
 * object_successes (nullable): row `row` of i32 [cap][G], the per-object success counts.
 * Launches: reduce, finish, and the copy when params / best_params are given and score_col >= 0.
 * DXRL_E_INVALID before any launch: null args or required pointer, G or K < 1, G K above
 * INT32_MAX, row outside [0, cap), score_col >= DXRL_PG_VAL_IS_BEST, patience < 0, params
 * without best_params or the reverse (or with num_params < 1), partial_doubles smaller than
 * dxrl_pg_val_partial_doubles(G, K).
 * ------------------------------------------------------------------------ */
#define DXRL_PG_VAL_COLS 16
enum dxrl_pg_val_col {
    DXRL_PG_VAL_ITERATION = 0,
    DXRL_PG_VAL_ENV_STEPS,
    DXRL_PG_VAL_TRAIN_ROW,
    DXRL_PG_VAL_EPISODES,
    DXRL_PG_VAL_SUCCESSES,
    DXRL_PG_VAL_SUCCESS_RATE,
    DXRL_PG_VAL_MEAN_RETURN,
    DXRL_PG_VAL_RETURN_STD,
    DXRL_PG_VAL_MEAN_LENGTH,
    DXRL_PG_VAL_MEAN_SUCCESS_LENGTH,
    DXRL_PG_VAL_MEAN_CONTACTS,
    DXRL_PG_VAL_MIN_OBJECT_SUCCESS_RATE,
    DXRL_PG_VAL_OBJECTS_SOLVED,
    DXRL_PG_VAL_EVAL_STATUS,
    DXRL_PG_VAL_IS_BEST,
    DXRL_PG_VAL_SINCE_BEST,
    DXRL_PG_VAL_NAMED /* 16 named columns == DXRL_PG_VAL_COLS (a multiple of 4) */
};

typedef struct dxrl_pg_val_header {
    int64_t rows_written;
    int64_t best_row;      /* -1: none yet */
    int64_t stopped_row;   /* -1: patience not exhausted */
    int64_t since_best;    /* the last written row's since_best */
    double best_score;     /* -inf: none yet */
    double reserved_f64[3];
} dxrl_pg_val_header;

typedef struct dxrl_pg_val_args {
    int64_t num_objects;             /* G                                                    */
    int64_t episodes_per_object;     /* K                                                    */
    int64_t row;                     /* table row this call writes, 0 <= row < cap           */
    int64_t cap;                     /* rows of the tables                                   */
    int64_t iteration;               /* column 0                                             */
    int64_t env_steps;               /* column 1                                             */
    int64_t train_row;               /* column 2                                             */
    int64_t num_params;              /* f32 elements of params / best_params                 */
    int64_t partial_doubles;         /* f64 elements of partial                              */
    int32_t score_col;               /* keep-best column, < 0: off                           */
    int32_t patience;                /* >= 0; 0: never stops                                 */
    double min_delta;                /* keep-best margin                                     */
    double solve_threshold;          /* objects_solved: success rate >= this                 */
    /* device inputs */
    const double*  ep_return;        /* f64 [E]                                              */
    const int32_t* ep_length;        /* i32 [E]                                              */
    const uint8_t* ep_success;       /* u8  [E]                                              */
    const uint8_t* ep_contacts;      /* u8  [E]                                              */
    const int32_t* status;           /* i32 [1] the episode kernel's status word             */
    const float*   params;           /* f32 [num_params] (nullable with best_params)         */
    /* device scratch and outputs */
    double*  partial;                /* f64 [partial_doubles] scratch                        */
    float*   best_params;            /* f32 [num_params] (nullable with params)              */
    double*  val;                    /* f64 [cap][DXRL_PG_VAL_COLS]                          */
    int32_t* object_successes;       /* i32 [cap][G] (nullable)                              */
    dxrl_pg_val_header* header;
} dxrl_pg_val_args;

/* f64 elements of dxrl_pg_val_row's `partial` scratch for G objects x K episodes. */
int dxrl_pg_val_partial_doubles(int64_t num_objects, int64_t episodes_per_object, int64_t* out);
int dxrl_pg_val_row(int32_t device, const dxrl_pg_val_args* args, void* stream);

/* ---------------------------------------------------------------------------
 * Noise-level validation row of a training run (csrc/dxrl_pg_val_levels.hip): dxrl_pg_val_row
 * over L noise levels of the same G objects x K episodes in one call.  The records are
 * level-major: level l, object o, episode k at (l G + o) K + k, E = L G K; level 0 is the
 * baseline.  One call writes row `row` of three tables and applies keep-best and patience to the
 * same dxrl_pg_val_header, by dxrl_pg_val_row's rules, on the selected score.
 *
 * val[row] (DXRL_PG_VAL_COLS columns): level 0's row, exactly what dxrl_pg_val_row writes for
 *   level 0's G K records; is_best / since_best follow the selected score.
 * levels[row][l] (DXRL_PG_VAL_LEVEL_COLS columns, enum dxrl_pg_val_level_col):
 *   obs_noise_std, dyn_noise_std     level_noise[l], copied
 *   episodes .. min_object_success_rate
 *                                    bit for bit the columns of those names dxrl_pg_val_row
 *                                    writes with its record pointers offset by l G K (the same
 *                                    1,024-record chunks, workgroups per level, merge order, and
 *                                    the moments' shift taken from the level's own first record)
 *   degradation                      success_rate[0] - success_rate[l]
 *   degradation_percentage           success_rate[0] > 0 ? degradation / success_rate[0] * 100
 *                                    : 0.0 (f64, in this order; both 0.0 for level 0)
 * robust[row] (DXRL_PG_VAL_ROBUST_COLS columns, enum dxrl_pg_val_robust_col; sums in level
 * order, then one division):
 *   levels                           L
 *   worst_level, worst_success_rate  the first minimum of success_rate over the levels
 *   mean_success_rate                over all levels
 *   mean_noisy_success_rate          over levels 1 .. L-1 (NaN when L == 1)
 *   max_degradation,                 maxima over the levels of the two degradation columns
 *   max_degradation_percentage
 *   worst_mean_return                minimum of mean_return over the levels
 * object_successes (nullable): i32 [cap][L][G].
 * Score: score_table 0 -> val[row][score_col], score_col < DXRL_PG_VAL_IS_BEST; score_table 1 ->
 * robust[row][score_col], score_col < DXRL_PG_VAL_ROBUST_COLS; score_col < 0: keep-best off.
 * Launches, whatever L: reduce (val_grid(G, K) workgroups x L), finish (one workgroup, one wave
 * per level), and the copy when params / best_params are given and score_col >= 0.  The same
 * inputs give the same bytes.
 * DXRL_E_INVALID before any launch: whatever dxrl_pg_val_row rejects, num_levels outside
 * [1, DXRL_PG_VAL_MAX_LEVELS], L G K above INT32_MAX, score_table outside {0, 1}, score_col
 * outside the selected table's score columns, null levels / robust / level_noise, partial_doubles
 * smaller than dxrl_pg_val_levels_partial_doubles(L, G, K).
 * ------------------------------------------------------------------------ */
#define DXRL_PG_VAL_MAX_LEVELS 16
#define DXRL_PG_VAL_LEVEL_COLS 12
enum dxrl_pg_val_level_col {
    DXRL_PG_VAL_LEVEL_OBS_NOISE_STD = 0,
    DXRL_PG_VAL_LEVEL_DYN_NOISE_STD,
    DXRL_PG_VAL_LEVEL_EPISODES,
    DXRL_PG_VAL_LEVEL_SUCCESSES,
    DXRL_PG_VAL_LEVEL_SUCCESS_RATE,
    DXRL_PG_VAL_LEVEL_MEAN_RETURN,
    DXRL_PG_VAL_LEVEL_RETURN_STD,
    DXRL_PG_VAL_LEVEL_MEAN_LENGTH,
    DXRL_PG_VAL_LEVEL_MEAN_CONTACTS,
    DXRL_PG_VAL_LEVEL_MIN_OBJECT_SUCCESS_RATE,
    DXRL_PG_VAL_LEVEL_DEGRADATION,
    DXRL_PG_VAL_LEVEL_DEGRADATION_PERCENTAGE,
    DXRL_PG_VAL_LEVEL_NAMED /* == DXRL_PG_VAL_LEVEL_COLS */
};
#define DXRL_PG_VAL_ROBUST_COLS 8
enum dxrl_pg_val_robust_col {
    DXRL_PG_VAL_ROBUST_LEVELS = 0,
    DXRL_PG_VAL_ROBUST_WORST_LEVEL,
    DXRL_PG_VAL_ROBUST_WORST_SUCCESS_RATE,
    DXRL_PG_VAL_ROBUST_MEAN_SUCCESS_RATE,
    DXRL_PG_VAL_ROBUST_MEAN_NOISY_SUCCESS_RATE,
    DXRL_PG_VAL_ROBUST_MAX_DEGRADATION,
    DXRL_PG_VAL_ROBUST_MAX_DEGRADATION_PERCENTAGE,
    DXRL_PG_VAL_ROBUST_WORST_MEAN_RETURN,
    DXRL_PG_VAL_ROBUST_NAMED /* == DXRL_PG_VAL_ROBUST_COLS */
};

typedef struct dxrl_pg_val_levels_args {
    int64_t num_objects;             /* G                                                    */
    int64_t episodes_per_object;     /* K                                                    */
    int64_t row;                     /* table row this call writes, 0 <= row < cap           */
    int64_t cap;                     /* rows of the tables                                   */
    int64_t iteration;               /* val column 0                                         */
    int64_t env_steps;               /* val column 1                                         */
    int64_t train_row;               /* val column 2                                         */
    int64_t num_params;              /* f32 elements of params / best_params                 */
    int64_t partial_doubles;         /* f64 elements of partial                              */
    int32_t score_col;               /* keep-best column of the selected table, < 0: off     */
    int32_t patience;                /* >= 0; 0: never stops                                 */
    double min_delta;                /* keep-best margin                                     */
    double solve_threshold;          /* objects_solved of the main row                       */
    int32_t num_levels;              /* L, 1 .. DXRL_PG_VAL_MAX_LEVELS                       */
    int32_t score_table;             /* 0: score_col indexes val[row], 1: robust[row]        */
    /* device inputs */
    const double*  ep_return;        /* f64 [L G K]                                          */
    const int32_t* ep_length;        /* i32 [L G K]                                          */
    const uint8_t* ep_success;       /* u8  [L G K]                                          */
    const uint8_t* ep_contacts;      /* u8  [L G K]                                          */
    const int32_t* status;           /* i32 [1] the episode kernel's status word             */
    const float*   params;           /* f32 [num_params] (nullable with best_params)         */
    const double*  level_noise;      /* f64 [L][2] obs std, dyn std                          */
    /* device scratch and outputs */
    double*  partial;                /* f64 [partial_doubles] scratch                        */
    float*   best_params;            /* f32 [num_params] (nullable with params)              */
    double*  val;                    /* f64 [cap][DXRL_PG_VAL_COLS]                          */
    double*  levels;                 /* f64 [cap][L][DXRL_PG_VAL_LEVEL_COLS]                 */
    double*  robust;                 /* f64 [cap][DXRL_PG_VAL_ROBUST_COLS]                   */
    int32_t* object_successes;       /* i32 [cap][L][G] (nullable)                           */
    dxrl_pg_val_header* header;
} dxrl_pg_val_levels_args;

/* f64 elements of dxrl_pg_val_levels_row's `partial` scratch for L levels of G objects x K episodes. */
int dxrl_pg_val_levels_partial_doubles(int32_t num_levels, int64_t num_objects, int64_t episodes_per_object,
                                       int64_t* out);
int dxrl_pg_val_levels_row(int32_t device, const dxrl_pg_val_levels_args* args, void* stream);

/* ---------------------------------------------------------------------------
 * Paired rows of a noise-level validation run with common random numbers
 * (csrc/dxrl_pg_val_paired.hip).  Enqueued behind dxrl_pg_val_levels_row on the same stream, on
 * the same level-major records, when the episode launch ran with
 * dxrl_eval_args.stream_period = G K: episode i of every level is then the same spawn, the same
 * standard normals and the same action noise, and only the level's noise scale differs.  It reads
 * the records and writes two tables of its own; the header, the three tables of
 * dxrl_pg_val_levels_row and keep-best are not touched.
 *
 * For level l, pair i in [0, G K) is (record l G K + i, record i); s0 / sl are the two success
 * flags (non-zero ep_success bytes), d_i = ep_return[l G K + i] - ep_return[i], n = G K.
 * paired[row][l] (DXRL_PG_VAL_PAIRED_COLS columns, enum dxrl_pg_val_paired_col):
 *   pairs                       n
 *   lost, gained                pairs with s0 and not sl; with sl and not s0
 *   both_success, both_fail     pairs with s0 and sl; with neither
 *   mean_return_diff            mean of d
 *   return_diff_std             sqrt(M2 / n), M2 the sum of squared deviations of d
 *   return_diff_stderr          sqrt(M2 / (n (n - 1))), NaN for n = 1
 *   mean_length_diff            (sum of ep_length[l G K + i] - ep_length[i], an exact integer) / n
 *   paired_degradation          (lost - gained) / n
 *   paired_degradation_stderr   with dn = (double)(lost - gained), dc = (double)(lost + gained),
 *                               N = (double)n, in f64 and in this order: q = dn * dn; q = q / N;
 *                               v = dc - q; v = v / N; v = v > 0 ? v : 0; sqrt(v) / sqrt(N)
 *   mcnemar                     dc > 0 ? (dn * dn) / dc : 0
 *   objects_with_loss           objects o with object_lost[o] > 0
 *   max_object_lost             the largest object_lost[o]
 * object_lost (nullable): i32 [cap][L][G], row `row`: lost pairs of each object (object o holds
 * pairs o K .. o K + K - 1).
 * Level 0 is paired with itself by the same code: zeros, and NaN where n = 1 says so.
 *
 * Integer columns are exact.  The moments of d are (count, mean, M2) triples of d - d_0 (d_0 the
 * level's first difference), each pair entering by merge(m, {1, d - d_0, 0}), merged in
 * dxrl_pg_val_row's fixed order (the same 1,024-pair chunks, four consecutive pairs per thread,
 * lanes by shuffles, waves and workgroup partials in index order).  Two launches whatever L is:
 * reduce (val_grid(G, K) workgroups x L), finish (one workgroup, one wave per level).  No
 * floating-point atomics; the same inputs give the same bytes.
 * DXRL_E_INVALID before any launch, outputs untouched: null args or required pointer (the records,
 * partial, paired), L outside [1, DXRL_PG_VAL_MAX_LEVELS], G or K < 1, L G K above INT32_MAX, row
 * outside [0, cap), partial_doubles smaller than dxrl_pg_val_paired_partial_doubles(L, G, K).
 * ------------------------------------------------------------------------ */
#define DXRL_PG_VAL_PAIRED_COLS 14
enum dxrl_pg_val_paired_col {
    DXRL_PG_VAL_PAIRED_PAIRS = 0,
    DXRL_PG_VAL_PAIRED_LOST,
    DXRL_PG_VAL_PAIRED_GAINED,
    DXRL_PG_VAL_PAIRED_BOTH_SUCCESS,
    DXRL_PG_VAL_PAIRED_BOTH_FAIL,
    DXRL_PG_VAL_PAIRED_MEAN_RETURN_DIFF,
    DXRL_PG_VAL_PAIRED_RETURN_DIFF_STD,
    DXRL_PG_VAL_PAIRED_RETURN_DIFF_STDERR,
    DXRL_PG_VAL_PAIRED_MEAN_LENGTH_DIFF,
    DXRL_PG_VAL_PAIRED_DEGRADATION,
    DXRL_PG_VAL_PAIRED_DEGRADATION_STDERR,
    DXRL_PG_VAL_PAIRED_MCNEMAR,
    DXRL_PG_VAL_PAIRED_OBJECTS_WITH_LOSS,
    DXRL_PG_VAL_PAIRED_MAX_OBJECT_LOST,
    DXRL_PG_VAL_PAIRED_NAMED /* == DXRL_PG_VAL_PAIRED_COLS */
};

typedef struct dxrl_pg_val_paired_args {
    int64_t num_objects;             /* G                                                    */
    int64_t episodes_per_object;     /* K                                                    */
    int64_t row;                     /* table row this call writes, 0 <= row < cap           */
    int64_t cap;                     /* rows of the tables                                   */
    int64_t partial_doubles;         /* f64 elements of partial                              */
    int32_t num_levels;              /* L, 1 .. DXRL_PG_VAL_MAX_LEVELS                       */
    int32_t reserved;
    /* device inputs */
    const double*  ep_return;        /* f64 [L G K]                                          */
    const int32_t* ep_length;        /* i32 [L G K]                                          */
    const uint8_t* ep_success;       /* u8  [L G K]                                          */
    /* device scratch and outputs */
    double*  partial;                /* f64 [partial_doubles] scratch (its own, not the levels row's) */
    double*  paired;                 /* f64 [cap][L][DXRL_PG_VAL_PAIRED_COLS]                */
    int32_t* object_lost;            /* i32 [cap][L][G] (nullable)                           */
} dxrl_pg_val_paired_args;

/* f64 elements of dxrl_pg_val_paired_row's `partial` scratch for L levels of G objects x K episodes. */
int dxrl_pg_val_paired_partial_doubles(int32_t num_levels, int64_t num_objects, int64_t episodes_per_object,
                                       int64_t* out);
int dxrl_pg_val_paired_row(int32_t device, const dxrl_pg_val_paired_args* args, void* stream);

/* ---------------------------------------------------------------------------
 * Failure-mode rows of a validation run (csrc/dxrl_pg_val_failure.hip): how the live actor fails,
 * per noise level.  Enqueued last on the validation's stream, behind dxrl_pg_val_row or
 * dxrl_pg_val_levels_row (and dxrl_pg_val_paired_row when that runs), on the same level-major
 * records plus the five history words of every episode (dxrl_eval_args.hist_moments: S1, S2,
 * first-five sum F, last-five sum L, peak).  A validation without noise levels is L = 1.  It reads
 * the records and writes tables of its own; the header, the tables of the other rows and keep-best
 * are not touched.
 *
 * Every episode is classified by the rules of dxrl_failure_summarize above (one statement of
 * them, csrc/dxrl_failure_rules.h) in its hist_moments form: n = ep_length clamped to
 * [0, max_steps], timeout_steps the bound of rule 1, and a tie row is included as the exact
 * comparison decides.  Its class is 0 for a success and 1 + m for failure mode m (list(FailureMode)
 * order, as ep_mode has it).
 *
 * failure_modes[row][l][m] (DXRL_PG_VAL_FAILURE_MODE_COLS columns, enum dxrl_pg_val_failure_mode_col),
 * formed in f64 from exact integer sums over the episodes of mode m in level l: c their number,
 * S1 / S2 the sums of ep_length and its square, C1 the sum of ep_contacts, F the failures of the
 * level, n = G K:
 *   count                 c
 *   frequency             F > 0 ? c / F : 0
 *   episode_share         c / n
 *   mean_episode_length   c > 0 ? S1 / c : 0
 *   std_episode_length    c > 0 ? sqrt((double)(c S2 - S1 S1) / (double)(c c)) : 0, the integer
 *                         expressions in i64 (np.std; exactly 0 when all lengths are equal)
 *   mean_final_contacts   c > 0 ? C1 / c : 0
 *   mean_confidence       c > 0 ? (sum of the confidences) / c : 0
 *   objects               objects with at least one episode of this mode (object o holds records
 *                         o K .. o K + K - 1 of the level)
 *   max_object_count      the most episodes of this mode one object has
 *   worst_object          the first object with that count, -1 when c = 0
 * failure_levels[row][l] (DXRL_PG_VAL_FAILURE_LEVEL_COLS columns, enum dxrl_pg_val_failure_level_col):
 *   episodes n, failures F, failure_rate F / n, dominant_mode (the first mode with the largest
 *   count, -1 when F = 0), dominant_frequency (F > 0 ? that count / F : 0), modes_present (modes
 *   with c > 0), tie_rows, mean_confidence (F > 0 ? (the six modes' confidence sums added in mode
 *   order) / F : 0).
 * failure_transitions i32 [cap][L][7][7] (nullable; written only when `paired` is set, which needs
 * the episode launch to have run with stream_period = G K): entry [l][from][to] counts the pairs i
 * whose baseline record i has class `from` and whose record l G K + i has class `to`.  Level 0 is
 * paired with itself, so its table is diagonal.  Exact.
 *
 * With c S2 < 2^62 the i64 expression cannot overflow: ep_length <= max_steps <=
 * DXRL_SUMMARY_MAX_STEPS asks for G K <= DXRL_PG_VAL_FAILURE_MAX_EPISODES.  The integer sums are
 * exact in any order.  The confidence sum is a float sum in dxrl_pg_val_row's fixed order: four
 * consecutive records per thread, lanes by shuffles, waves and workgroup partials in index order.
 * Two launches whatever L is: reduce (val_grid(G, K) workgroups x L), finish (one workgroup, one
 * wave per level).  No floating-point atomics; the same inputs give the same bytes.
 * DXRL_E_INVALID before any launch, outputs untouched: null args or required pointer (the records,
 * hist_moments, partial, failure_modes, failure_levels), L outside [1, DXRL_PG_VAL_MAX_LEVELS], G or
 * K < 1, L G K above INT32_MAX, G K above DXRL_PG_VAL_FAILURE_MAX_EPISODES, max_steps outside
 * [1, DXRL_SUMMARY_MAX_STEPS], timeout_steps < 1, row outside [0, cap), partial_doubles smaller than
 * dxrl_pg_val_failure_partial_doubles(L, G, K), paired set with a null failure_transitions.
 * ------------------------------------------------------------------------ */
#define DXRL_PG_VAL_FAILURE_MAX_EPISODES (1 << 19) /* G K above it -> DXRL_E_INVALID */
#define DXRL_PG_VAL_FAILURE_CLASSES 7               /* success, then the DXRL_FAILURE_MODES modes */
#define DXRL_PG_VAL_FAILURE_MODE_COLS 10
enum dxrl_pg_val_failure_mode_col {
    DXRL_PG_VAL_FAILURE_COUNT = 0,
    DXRL_PG_VAL_FAILURE_FREQUENCY,
    DXRL_PG_VAL_FAILURE_EPISODE_SHARE,
    DXRL_PG_VAL_FAILURE_MEAN_EPISODE_LENGTH,
    DXRL_PG_VAL_FAILURE_STD_EPISODE_LENGTH,
    DXRL_PG_VAL_FAILURE_MEAN_FINAL_CONTACTS,
    DXRL_PG_VAL_FAILURE_MEAN_CONFIDENCE,
    DXRL_PG_VAL_FAILURE_OBJECTS,
    DXRL_PG_VAL_FAILURE_MAX_OBJECT_COUNT,
    DXRL_PG_VAL_FAILURE_WORST_OBJECT,
    DXRL_PG_VAL_FAILURE_MODE_NAMED /* == DXRL_PG_VAL_FAILURE_MODE_COLS */
};
#define DXRL_PG_VAL_FAILURE_LEVEL_COLS 8
enum dxrl_pg_val_failure_level_col {
    DXRL_PG_VAL_FAILURE_LEVEL_EPISODES = 0,
    DXRL_PG_VAL_FAILURE_LEVEL_FAILURES,
    DXRL_PG_VAL_FAILURE_LEVEL_FAILURE_RATE,
    DXRL_PG_VAL_FAILURE_LEVEL_DOMINANT_MODE,
    DXRL_PG_VAL_FAILURE_LEVEL_DOMINANT_FREQUENCY,
    DXRL_PG_VAL_FAILURE_LEVEL_MODES_PRESENT,
    DXRL_PG_VAL_FAILURE_LEVEL_TIE_ROWS,
    DXRL_PG_VAL_FAILURE_LEVEL_MEAN_CONFIDENCE,
    DXRL_PG_VAL_FAILURE_LEVEL_NAMED /* == DXRL_PG_VAL_FAILURE_LEVEL_COLS */
};

typedef struct dxrl_pg_val_failure_args {
    int64_t num_objects;             /* G                                                    */
    int64_t episodes_per_object;     /* K                                                    */
    int64_t row;                     /* table row this call writes, 0 <= row < cap           */
    int64_t cap;                     /* rows of the tables                                   */
    int64_t partial_doubles;         /* f64 elements of partial                              */
    int32_t num_levels;              /* L, 1 .. DXRL_PG_VAL_MAX_LEVELS                       */
    int32_t paired;                  /* 0 / 1: write failure_transitions                     */
    int32_t max_steps;               /* the history bound n is clamped to (1 .. DXRL_SUMMARY_MAX_STEPS) */
    int32_t timeout_steps;           /* the timeout bound of rule 1                          */
    int32_t success_threshold;       /* rule 6                                               */
    int32_t reserved;
    /* device inputs */
    const int32_t* ep_length;        /* i32 [L G K]                                          */
    const uint8_t* ep_success;       /* u8  [L G K]                                          */
    const uint8_t* ep_contacts;      /* u8  [L G K]                                          */
    const int32_t* hist_moments;     /* i32 [L G K][5] S1, S2, F, L, peak                    */
    /* device scratch and outputs */
    double*  partial;                /* f64 [partial_doubles] scratch (its own)              */
    double*  failure_modes;          /* f64 [cap][L][6][DXRL_PG_VAL_FAILURE_MODE_COLS]       */
    double*  failure_levels;         /* f64 [cap][L][DXRL_PG_VAL_FAILURE_LEVEL_COLS]         */
    int32_t* failure_transitions;    /* i32 [cap][L][7][7] (nullable unless paired)          */
} dxrl_pg_val_failure_args;

/* f64 elements of dxrl_pg_val_failure_row's `partial` scratch for L levels of G objects x K episodes. */
int dxrl_pg_val_failure_partial_doubles(int32_t num_levels, int64_t num_objects, int64_t episodes_per_object,
                                        int64_t* out);
int dxrl_pg_val_failure_row(int32_t device, const dxrl_pg_val_failure_args* args, void* stream);

/* ---------------------------------------------------------------------------
 * A set of training runs reduced on the device (csrc/dxrl_pg_runs.hip): the layer above
 * one fit().  The runs' device tables -- training logs (cols = DXRL_PG_LOG_COLS) or
 * validation tables (cols = DXRL_PG_VAL_COLS), one call per slab -- lie in one slab
 *   tables f64 [R][cap][cols],  run_rows i32 [R] (rows written of every run),
 * and are reduced to per-run rows, per-group tables (CSR groups of runs, the semantics of
 * dxrl_study_summarize: group g holds group_runs[group_offsets[g] .. group_offsets[g+1]),
 * groups may overlap or be empty) and contrasts paired by member position.  At most three
 * launches on the caller's stream (run pass; group pass when G > 0; contrast pass when
 * Q > 0), no host synchronisation, no floating-point atomics: the same inputs give the
 * same bytes on every call.
 *
 * A spec s is (col, x_col, window W, threshold, final_window FW): the column the
 * statistics are taken of, the column reported at convergence, and dxrl_pg_log_row's
 * convergence rule.  S specs per call (1 .. DXRL_PG_RUNS_MAX_SPECS), read on the host.
 *
 * Run pass, a wavefront per (run, spec), n = run_rows[r], v_i = tables[r][i][col]:
 * run_table f64 [R][S][DXRL_PG_RUNS_RUN_COLS]:
 *   0 n
 *   1 final_window_mean: the left-to-right f64 sum of v_{n-k} .. v_{n-1}, k = min(FW, n),
 *     divided by k; NaN if one of them is NaN or n = 0
 *   2 best, 3 best_row: the maximum over the non-NaN rows, the first maximum wins;
 *     NaN / -1 if there is none
 *   4 convergence_row: dxrl_pg_log_row's rule -- the first row i >= W - 1 whose window mean
 *     (v_{i-W+1} + .. + v_i, summed oldest first in f64, divided by W) is strictly above
 *     threshold; a NaN in the window does not converge; -1 if no row does
 *   5 x_at_convergence: tables[r][convergence_row][x_col], NaN if not converged
 *   6 curve_mean: the sum of the non-NaN rows divided by their number (NaN if none).
 *     SUMMATION ORDER: wave lane t adds rows t, t + 64, t + 128, .. in ascending order to
 *     a partial that starts at 0.0 (a NaN row adds nothing); the 64 partials are added in
 *     the fixed tree p[t] += p[t + o] for o = 32, 16, 8, 4, 2, 1
 *   7 the number of NaN rows
 *
 * Group pass, a wavefront per (group, spec).  The five metrics of a run, in this order:
 * DXRL_PG_RUNS_FINAL_WINDOW_MEAN (column 1), _BEST (2), _CONVERGENCE_ROW (4; a run that
 * did not converge has no value), _X_AT_CONVERGENCE (5), _CURVE_MEAN (6).
 * group_table f64 [G][S][5][DXRL_PG_RUNS_GROUP_COLS], per metric over the group's runs
 * whose value is finite: 0 count, 1 mean, 2 population standard deviation (np.std), 3 min,
 * 4 max (1 .. 4 NaN when count = 0), 5 the number of the group's runs that converged
 * (column 4 >= 0; the same in all five rows).  ORDER: wave lane t takes members t, t + 64,
 * .. of the group in ascending position as Welford steps into a (count, mean, M2) triple;
 * the 64 triples are merged with Chan et al.'s update in the tree t[i] = merge(t[i],
 * t[i + o]) for o = 32, .., 1; std = sqrt(M2 / count).
 *
 * Contrast pass, a wavefront per (contrast, spec): contrast_weights f64 [Q][G].  The
 * groups with a non-zero weight in contrast q must have one member count m (else status
 * bit 2 and the contrast's rows are NaN).  For position j < m,
 *   d_j = sum over g, ascending, of w[q][g] * x[member j of g]     (w[q][g] != 0 only),
 * the products added left to right to 0.0: member j is the same seed in every arm, so a
 * pairwise difference is the weights (+1, -1), a main effect of a 2 x 2 (+-1/2) and the
 * interaction (+1 -1 -1 +1).  contrast_table f64 [Q][S][5][DXRL_PG_RUNS_CONTRAST_COLS],
 * per metric over the positions j whose every term is finite (an out-of-range member has
 * no finite value): 0 pairs n, 1 mean of d, 2 sample standard deviation (ddof 1, NaN for
 * n < 2), 3 standard error std / sqrt(n), 4 mean / standard error; 1 .. 4 are NaN when
 * n = 0.  ORDER: as the group pass, over positions.
 *
 * status i32 [1] (zeroed on the stream by the call): bit 0 = a group offset or member was
 * out of range (skipped: a group with bad offsets is an empty group; nothing is accessed
 * out of bounds); bit 1 = run_rows[r] outside [0, cap] (the run is treated as empty);
 * bit 2 = a contrast whose weighted groups differ in size, or one of which has bad offsets
 * (its rows are NaN).
 * DXRL_E_INVALID before any launch: null args or a null required pointer (tables,
 * run_rows, specs, run_table, status; group_offsets and group_table when G > 0,
 * group_runs when num_members > 0; contrast_weights and contrast_table when Q > 0);
 * R, cap, cols or S < 1; S > DXRL_PG_RUNS_MAX_SPECS; col or x_col outside [0, cols);
 * W or FW < 1; G, Q or num_members < 0; Q > 0 with G = 0.
 * ------------------------------------------------------------------------ */
#define DXRL_PG_RUNS_MAX_SPECS 16
#define DXRL_PG_RUNS_RUN_COLS 8
#define DXRL_PG_RUNS_METRICS 5
#define DXRL_PG_RUNS_GROUP_COLS 6
#define DXRL_PG_RUNS_CONTRAST_COLS 5
enum dxrl_pg_runs_run_col {
    DXRL_PG_RUNS_RUN_ROWS = 0,
    DXRL_PG_RUNS_RUN_FINAL_WINDOW_MEAN,
    DXRL_PG_RUNS_RUN_BEST,
    DXRL_PG_RUNS_RUN_BEST_ROW,
    DXRL_PG_RUNS_RUN_CONVERGENCE_ROW,
    DXRL_PG_RUNS_RUN_X_AT_CONVERGENCE,
    DXRL_PG_RUNS_RUN_CURVE_MEAN,
    DXRL_PG_RUNS_RUN_NAN_ROWS
};
enum dxrl_pg_runs_metric {
    DXRL_PG_RUNS_FINAL_WINDOW_MEAN = 0,
    DXRL_PG_RUNS_BEST,
    DXRL_PG_RUNS_CONVERGENCE_ROW,
    DXRL_PG_RUNS_X_AT_CONVERGENCE,
    DXRL_PG_RUNS_CURVE_MEAN
};

typedef struct dxrl_pg_runs_spec {
    int32_t col;                     /* the column the statistics are taken of              */
    int32_t x_col;                   /* the column reported at the convergence row          */
    int32_t window;                  /* W >= 1                                               */
    int32_t final_window;            /* FW >= 1                                              */
    double  threshold;
} dxrl_pg_runs_spec;

typedef struct dxrl_pg_runs_args {
    int32_t num_runs;                /* R                                                    */
    int32_t cap;                     /* rows of every run's table in the slab                */
    int32_t cols;                    /* f64 columns of a row                                 */
    int32_t num_specs;               /* S, 1 .. DXRL_PG_RUNS_MAX_SPECS                       */
    int32_t num_groups;              /* G (0 = no group pass)                                */
    int32_t num_members;             /* entries of group_runs (bounds check)                 */
    int32_t num_contrasts;           /* Q (0 = no contrast pass)                             */
    int32_t reserved;
    const dxrl_pg_runs_spec* specs;  /* HOST [S]                                             */
    /* device inputs */
    const double*  tables;           /* f64 [R][cap][cols]                                   */
    const int32_t* run_rows;         /* i32 [R]                                              */
    const int32_t* group_offsets;    /* i32 [G + 1] CSR offsets into group_runs              */
    const int32_t* group_runs;       /* i32 [num_members] runs (slab rows)                   */
    const double*  contrast_weights; /* f64 [Q][G]                                           */
    /* device outputs */
    double*  run_table;              /* f64 [R][S][8]                                        */
    double*  group_table;            /* f64 [G][S][5][6]                                     */
    double*  contrast_table;         /* f64 [Q][S][5][5]                                     */
    int32_t* status;                 /* i32 [1]                                              */
} dxrl_pg_runs_args;

int dxrl_pg_runs_summarize(int32_t device, const dxrl_pg_runs_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DXRL_H_ */
