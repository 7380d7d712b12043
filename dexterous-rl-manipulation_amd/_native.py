"""ctypes binding of libdxrl.so (the C ABI declared in include/dxrl.h).

The library is built in-tree by ``build.build_native()`` (hipcc, gfx950) and
loaded here.  There is no fallback: if the library is missing or no GPU is
visible, every product entry point raises.  torch is imported first so the
library binds to the HIP runtime torch already loaded (one runtime per
process; streams and device pointers are shared).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch  # noqa: F401  (loads libamdhip64 first; see module docstring)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DXRL_LIB") or os.path.join(PKG_DIR, "libdxrl.so")  # DXRL_LIB: A/B builds

DXRL_OK = 0
DXRL_E_INVALID = -1
DXRL_E_HIP = -2
DXRL_E_UNSUPPORTED = -3
DXRL_E_TAPE = -4
REWARD_SPARSE = 0
REWARD_DENSE = 1
RESET_EXTRA = 6
MAX_CURRICULA = 256
SUCCESS_TRAINING = 0
SUCCESS_TERMINATED = 1
ABI_VERSION = 1
EVAL_POLICY_SIMPLE = 0
EVAL_POLICY_HEURISTIC = 1
EVAL_POLICY_RANDOM = 2
EVAL_POLICY_MLP = 3


class Curriculum(C.Structure):
    _fields_ = [("object_size", C.c_double), ("object_mass", C.c_double), ("friction_coefficient", C.c_double),
                ("size_range", C.c_double * 2), ("mass_range", C.c_double * 2), ("friction_range", C.c_double * 2),
                ("spawn_x_range", C.c_double * 2), ("spawn_y_range", C.c_double * 2),
                ("spawn_z_range", C.c_double * 2),
                ("has_size_range", C.c_int32), ("has_mass_range", C.c_int32), ("has_friction_range", C.c_int32),
                ("friction_is_f64_scalar", C.c_int32)]


class EnvConfig(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("num_fingers", C.c_int32), ("joints_per_finger", C.c_int32),
                ("max_episode_steps", C.c_int32), ("reward_type", C.c_int32), ("has_object_position", C.c_int32),
                ("object_position", C.c_double * 3),
                ("distance_weight", C.c_double), ("contact_weight", C.c_double), ("closure_weight", C.c_double),
                ("stability_weight", C.c_double), ("seed", C.c_uint64), ("global_env_offset", C.c_int64)]


class EnvLayout(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("total_bytes", "jp", "jv", "op", "ov", "flags", "step_count", "size",
                                         "mass", "friction", "cfg_index", "reset_ctr", "curricula")]


class LearnerLayout(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("total_bytes", "mean", "best", "ep_return", "noise_ctr")]


class LearnerConfig(C.Structure):
    _fields_ = [("learning_rate", C.c_double), ("exploration_noise", C.c_double),
                ("action_clip_range", C.c_double), ("seed", C.c_uint64)]


class RolloutIO(C.Structure):
    _fields_ = [("gauss", C.c_void_p), ("gauss_stride", C.c_int64), ("reset_draws", C.c_void_p),
                ("reset_stride", C.c_int64), ("record_cap", C.c_int32), ("ep_return", C.c_void_p),
                ("ep_length", C.c_void_p), ("ep_success", C.c_void_p), ("ep_end_step", C.c_void_p),
                ("ep_count", C.c_void_p), ("gauss_used", C.c_void_p), ("status", C.c_void_p),
                ("episode_budget", C.c_void_p)]


STUDY_MAX_GROUPS = 16      # DXRL_STUDY_MAX_GROUPS
STUDY_MAX_MILESTONES = 64  # DXRL_STUDY_MAX_MILESTONES
STUDY_FIXED, STUDY_SUCCESS_WINDOW, STUDY_STEP_MILESTONES = 0, 1, 2


class StudyGroup(C.Structure):
    _fields_ = [("mode", C.c_int32), ("window", C.c_int32), ("min_successes", C.c_int32),
                ("num_levels", C.c_int32), ("first_row", C.c_int32), ("num_milestones", C.c_int32),
                ("min_episodes", C.c_int64), ("milestones", C.c_int64 * STUDY_MAX_MILESTONES)]


class StudyLayout(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("total_bytes", "window_mask", "total_steps", "total_episodes", "level",
                                         "milestone")]


class StudyArgs(C.Structure):
    _fields_ = [("groups", C.c_void_p), ("num_groups", C.c_int32), ("lane_group", C.c_void_p),
                ("sched_state", C.c_void_p), ("ep_level", C.c_void_p), ("lane_stream", C.c_void_p)]


class PgRolloutArgs(C.Structure):
    _fields_ = [("horizon", C.c_int32), ("max_steps", C.c_int32), ("policy_seed", C.c_uint64),
                ("iteration", C.c_uint64), ("obs_noise_std", C.c_double), ("dyn_noise_std", C.c_double)] + \
               [(k, C.c_void_p) for k in ("obs_rm", "obs_fm", "act", "logp", "rew", "done", "ep_return", "ep_count",
                                          "ep_sum_return", "ep_sum_length", "ep_successes")] + \
               [("diag_flags", C.c_int32), ("success_rule", C.c_int32), ("record_cap", C.c_int32),
                ("rec_return", C.c_void_p), ("rec_length", C.c_void_p), ("rec_success", C.c_void_p),
                ("rec_end_step", C.c_void_p), ("ep_code", C.c_void_p), ("applied_act", C.c_void_p),
                ("dyn_noise_tape", C.c_void_p), ("obs_noise_tape", C.c_void_p), ("h2_tape", C.c_void_p)]


class PgHeadsArgs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("mu", "values", "act", "logp_old", "adv", "ret", "stats", "params")] + \
               [("num_samples", C.c_int64), ("inv_total_samples", C.c_double), ("clip_eps", C.c_double),
                ("vf_coef", C.c_double), ("ent_coef", C.c_double)] + \
               [(k, C.c_void_p) for k in ("dmu_rm", "dmu_fm", "dv_rm", "dv_fm", "dlogstd_partial", "loss_partial",
                                          "grads")]


class PgFusedArgs(C.Structure):
    _fields_ = [("net", C.c_int32), ("train", C.c_int32), ("rows", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("packed", "params", "obs", "act", "logp_old", "adv", "ret", "stats")] + \
               [(k, C.c_double) for k in ("inv_total_samples", "clip_eps", "vf_coef", "ent_coef")] + \
               [(k, C.c_void_p) for k in ("values", "h1", "dh2", "partial", "loss_partial")] + \
               [("grid", C.c_int32), ("wgrad_splits", C.c_int32), ("wgrad_partial", C.c_void_p),
                ("grads", C.c_void_p), ("h1_mode", C.c_int32), ("h2_in", C.c_void_p), ("h2_out", C.c_void_p)]


class SchedArgs(C.Structure):
    _fields_ = [("codes", C.c_void_p), ("world", C.c_int32), ("horizon", C.c_int32), ("num_envs", C.c_int64),
                ("window", C.c_int32), ("max_candidates", C.c_int32), ("threshold", C.c_double),
                ("min_episodes", C.c_int64), ("episodes_before", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("tail_in", "tail_len_in", "tail_out", "tail_len_out", "scratch")] + \
               [("scratch_bytes", C.c_int64), ("summary", C.c_void_p)]


class SchedPackedArgs(C.Structure):
    _fields_ = [("packs", C.c_void_p), ("pack_words", C.c_int64), ("bits", C.c_int32), ("world", C.c_int32),
                ("horizon", C.c_int32), ("num_envs", C.c_int64), ("window", C.c_int32),
                ("max_candidates", C.c_int32), ("threshold", C.c_double), ("min_episodes", C.c_int64),
                ("episodes_before", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("tail_in", "tail_len_in", "tail_out", "tail_len_out", "scratch")] + \
               [("scratch_bytes", C.c_int64), ("summary", C.c_void_p), ("where", C.c_void_p)]


SCHED_MAX_CANDIDATES = 64  # DXRL_SCHED_MAX_CANDIDATES


class EvalSegment(C.Structure):
    _fields_ = [("curriculum_row", C.c_int32), ("num_episodes", C.c_int32), ("first_episode", C.c_int32),
                ("reserved", C.c_int32), ("obs_noise_std", C.c_double), ("dyn_noise_std", C.c_double),
                ("noise_offset", C.c_int64), ("noise_count", C.c_int64)]


class EvalArgs(C.Structure):
    _fields_ = [("num_lanes", C.c_int32), ("policy", C.c_int32), ("max_steps", C.c_int32),
                ("total_episodes", C.c_int32), ("lane_segments", C.c_void_p), ("segments", C.c_void_p),
                ("mean_action", C.c_void_p), ("exploration_noise", C.c_double), ("policy_tape", C.c_void_p),
                ("policy_stride", C.c_int64), ("noise_tape", C.c_void_p), ("reset_tape", C.c_void_p),
                ("policy_seed", C.c_uint64), ("noise_seed", C.c_uint64), ("reset_seed", C.c_uint64),
                ("stream_period", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("ep_return", "ep_length", "ep_success", "ep_contacts", "contact_hist",
                                          "policy_used", "status", "obs_traj", "act_traj", "work_queue",
                                          "hist_moments")]


class EvalMlp(C.Structure):
    _fields_ = [("packed", C.c_void_p), ("params", C.c_void_p), ("action_std", C.c_void_p)]


SUMMARY_MAX_STEPS = 4096  # DXRL_SUMMARY_MAX_STEPS (metrics._EXACT_VAR_MAX_N)


class EvalSummaryArgs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("total_episodes", "max_steps", "success_threshold", "num_groups",
                                         "num_members", "tie_cap")] + \
               [(k, C.c_void_p) for k in ("ep_length", "ep_success", "ep_contacts", "ep_return", "contact_hist",
                                          "group_offsets", "group_episodes", "ep_work", "ep_code", "ep_moments",
                                          "group_stats", "group_return", "tie_count", "tie_list", "status")]


FAILURE_MODES = 6  # DXRL_FAILURE_MODES


class FailureSummaryArgs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("total_episodes", "max_steps", "timeout_steps", "success_threshold",
                                         "num_groups", "num_members", "tie_cap", "reserved")] + \
               [(k, C.c_void_p) for k in ("ep_length", "ep_success", "ep_contacts", "ep_props", "contact_hist",
                                          "hist_moments", "group_offsets", "group_episodes", "ep_work", "ep_mode",
                                          "ep_confidence", "mode_stats", "group_totals", "mode_props", "tie_count",
                                          "tie_list", "status")]


class RobustnessSummaryArgs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("total_episodes", "max_steps", "success_threshold", "num_groups",
                                         "num_members", "tie_cap")] + \
               [(k, C.c_void_p) for k in ("ep_length", "ep_success", "ep_contacts", "ep_return", "hist_moments",
                                          "group_offsets", "group_episodes", "baseline_group", "group_stats",
                                          "group_return", "level_table", "ep_code", "tie_count", "tie_list",
                                          "status")]


STUDY_LANE_INTS, STUDY_LANE_REALS, STUDY_METRICS = 8, 4, 5  # DXRL_STUDY_LANE_INTS / _LANE_REALS / _METRICS


class StudySummaryArgs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("num_lanes", "record_cap", "lane_offset", "total_lanes", "window",
                                         "min_count", "num_groups", "num_members", "tie_cap", "reserved")] + \
               [("reward_threshold", C.c_double)] + \
               [(k, C.c_void_p) for k in ("ep_return", "ep_length", "ep_success", "ep_level", "lane_episodes",
                                          "group_offsets", "group_lanes", "lane_ints", "lane_reals", "group_stats",
                                          "group_metrics", "tie_count", "tie_list", "status")]


# enum dxrl_pg_log_col: the named columns of the training log, in table order
PG_LOG_COLUMNS = ("iteration", "env_steps", "episodes", "mean_return", "mean_length", "success_rate",
                  "mean_step_reward", "done_fraction", "value_mean", "target_mean", "target_var", "residual_var",
                  "explained_variance", "adv_mean", "adv_std", "policy_loss", "value_mse", "clip_frac", "approx_kl",
                  "grad_norm", "is_best", "window_mean")
PG_LOG_NAMED = len(PG_LOG_COLUMNS)  # DXRL_PG_LOG_NAMED
PG_LOG_COLS = 24                    # DXRL_PG_LOG_COLS
PG_LOG_IS_BEST = PG_LOG_COLUMNS.index("is_best")
# enum dxrl_pg_log_rank_col: the named entries of a rank record (dxrl_pg_log_rank_pack), in order
PG_LOG_RANK_COLUMNS = ("samples", "reward_sum", "value_sum", "done_count", "target_mean", "target_m2",
                       "residual_mean", "residual_m2", "episodes", "length_sum", "successes", "return_sum",
                       "policy_loss_sum", "value_se_sum", "clip_sum", "kl_sum", "loss_rows")
PG_LOG_RANK_NAMED = len(PG_LOG_RANK_COLUMNS)  # DXRL_PG_LOG_RANK_NAMED
PG_LOG_RANK_DOUBLES = 20                      # DXRL_PG_LOG_RANK_DOUBLES


class PgLogHeader(C.Structure):
    _fields_ = [("rows_written", C.c_int64), ("best_row", C.c_int64), ("converged_row", C.c_int64),
                ("reserved", C.c_int64), ("best_score", C.c_double), ("reserved_f64", C.c_double * 3)]


class PgLogArgs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("num_envs", "horizon", "row", "cap", "iteration", "env_steps", "loss_blocks",
                                         "loss_rows", "min_episodes", "num_params", "partial_doubles")] + \
               [(k, C.c_int32) for k in ("score_col", "conv_col", "conv_window", "reserved")] + \
               [("conv_threshold", C.c_double)] + \
               [(k, C.c_void_p) for k in ("ep_count", "ep_sum_return", "ep_sum_length", "ep_successes", "rew", "ret",
                                          "done", "values", "stats", "loss_partial", "gnorm2", "params", "partial",
                                          "best_params", "log", "header")]


# enum dxrl_pg_val_col: the named columns of the validation table, in table order
PG_VAL_COLUMNS = ("iteration", "env_steps", "train_row", "episodes", "successes", "success_rate", "mean_return",
                  "return_std", "mean_length", "mean_success_length", "mean_contacts", "min_object_success_rate",
                  "objects_solved", "eval_status", "is_best", "since_best")
PG_VAL_NAMED = len(PG_VAL_COLUMNS)  # DXRL_PG_VAL_NAMED
PG_VAL_COLS = 16                    # DXRL_PG_VAL_COLS
PG_VAL_IS_BEST = PG_VAL_COLUMNS.index("is_best")


class PgValHeader(C.Structure):
    _fields_ = [("rows_written", C.c_int64), ("best_row", C.c_int64), ("stopped_row", C.c_int64),
                ("since_best", C.c_int64), ("best_score", C.c_double), ("reserved_f64", C.c_double * 3)]


class PgValArgs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("num_objects", "episodes_per_object", "row", "cap", "iteration", "env_steps",
                                         "train_row", "num_params", "partial_doubles")] + \
               [("score_col", C.c_int32), ("patience", C.c_int32), ("min_delta", C.c_double),
                ("solve_threshold", C.c_double)] + \
               [(k, C.c_void_p) for k in ("ep_return", "ep_length", "ep_success", "ep_contacts", "status", "params",
                                          "partial", "best_params", "val", "object_successes", "header")]


# enum dxrl_pg_val_level_col / dxrl_pg_val_robust_col: the per-level and over-levels tables of
# dxrl_pg_val_levels_row, in table order
PG_VAL_MAX_LEVELS = 16              # DXRL_PG_VAL_MAX_LEVELS
PG_VAL_LEVEL_COLUMNS = ("obs_noise_std", "dyn_noise_std", "episodes", "successes", "success_rate", "mean_return",
                        "return_std", "mean_length", "mean_contacts", "min_object_success_rate", "degradation",
                        "degradation_percentage")
PG_VAL_LEVEL_COLS = len(PG_VAL_LEVEL_COLUMNS)    # DXRL_PG_VAL_LEVEL_COLS
PG_VAL_ROBUST_COLUMNS = ("levels", "worst_level", "worst_success_rate", "mean_success_rate",
                         "mean_noisy_success_rate", "max_degradation", "max_degradation_percentage",
                         "worst_mean_return")
PG_VAL_ROBUST_COLS = len(PG_VAL_ROBUST_COLUMNS)  # DXRL_PG_VAL_ROBUST_COLS


class PgValLevelsArgs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("num_objects", "episodes_per_object", "row", "cap", "iteration", "env_steps",
                                         "train_row", "num_params", "partial_doubles")] + \
               [("score_col", C.c_int32), ("patience", C.c_int32), ("min_delta", C.c_double),
                ("solve_threshold", C.c_double), ("num_levels", C.c_int32), ("score_table", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("ep_return", "ep_length", "ep_success", "ep_contacts", "status", "params",
                                          "level_noise", "partial", "best_params", "val", "levels", "robust",
                                          "object_successes", "header")]


# enum dxrl_pg_val_paired_col: the per-level paired table of dxrl_pg_val_paired_row, in table order
PG_VAL_PAIRED_COLUMNS = ("pairs", "lost", "gained", "both_success", "both_fail", "mean_return_diff",
                         "return_diff_std", "return_diff_stderr", "mean_length_diff", "paired_degradation",
                         "paired_degradation_stderr", "mcnemar", "objects_with_loss", "max_object_lost")
PG_VAL_PAIRED_COLS = len(PG_VAL_PAIRED_COLUMNS)  # DXRL_PG_VAL_PAIRED_COLS


class PgValPairedArgs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("num_objects", "episodes_per_object", "row", "cap", "partial_doubles")] + \
               [("num_levels", C.c_int32), ("reserved", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("ep_return", "ep_length", "ep_success", "partial", "paired", "object_lost")]


# enum dxrl_pg_val_failure_mode_col / dxrl_pg_val_failure_level_col: the failure tables of
# dxrl_pg_val_failure_row, in table order; the classes of its transitions (success, then the modes)
PG_VAL_FAILURE_MAX_EPISODES = 1 << 19  # DXRL_PG_VAL_FAILURE_MAX_EPISODES
PG_VAL_FAILURE_CLASSES = FAILURE_MODES + 1  # DXRL_PG_VAL_FAILURE_CLASSES
PG_VAL_FAILURE_MODE_COLUMNS = ("count", "frequency", "episode_share", "mean_episode_length", "std_episode_length",
                               "mean_final_contacts", "mean_confidence", "objects", "max_object_count",
                               "worst_object")
PG_VAL_FAILURE_MODE_COLS = len(PG_VAL_FAILURE_MODE_COLUMNS)    # DXRL_PG_VAL_FAILURE_MODE_COLS
PG_VAL_FAILURE_LEVEL_COLUMNS = ("episodes", "failures", "failure_rate", "dominant_mode", "dominant_frequency",
                                "modes_present", "tie_rows", "mean_confidence")
PG_VAL_FAILURE_LEVEL_COLS = len(PG_VAL_FAILURE_LEVEL_COLUMNS)  # DXRL_PG_VAL_FAILURE_LEVEL_COLS


class PgValFailureArgs(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("num_objects", "episodes_per_object", "row", "cap", "partial_doubles")] + \
               [(k, C.c_int32) for k in ("num_levels", "paired", "max_steps", "timeout_steps", "success_threshold",
                                         "reserved")] + \
               [(k, C.c_void_p) for k in ("ep_length", "ep_success", "ep_contacts", "hist_moments", "partial",
                                          "failure_modes", "failure_levels", "failure_transitions")]


# dxrl_pg_runs_summarize: a set of runs' tables reduced to run rows, group tables and contrasts
PG_RUNS_MAX_SPECS = 16  # DXRL_PG_RUNS_MAX_SPECS
# enum dxrl_pg_runs_run_col: the columns of a run row, in table order
PG_RUNS_RUN_COLUMNS = ("rows", "final_window_mean", "best", "best_row", "convergence_row", "x_at_convergence",
                       "curve_mean", "nan_rows")
PG_RUNS_RUN_COLS = len(PG_RUNS_RUN_COLUMNS)  # DXRL_PG_RUNS_RUN_COLS
# enum dxrl_pg_runs_metric: the metrics of the group and contrast tables, in table order
PG_RUNS_METRICS = ("final_window_mean", "best", "convergence_row", "x_at_convergence", "curve_mean")
PG_RUNS_GROUP_COLUMNS = ("count", "mean", "std", "min", "max", "num_converged")  # DXRL_PG_RUNS_GROUP_COLS
PG_RUNS_CONTRAST_COLUMNS = ("pairs", "mean", "std", "stderr", "t")              # DXRL_PG_RUNS_CONTRAST_COLS
PG_RUNS_ST_RANGE, PG_RUNS_ST_ROWS, PG_RUNS_ST_CONTRAST = 1, 2, 4


class PgRunsSpec(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("col", "x_col", "window", "final_window")] + [("threshold", C.c_double)]


class PgRunsArgs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("num_runs", "cap", "cols", "num_specs", "num_groups", "num_members",
                                         "num_contrasts", "reserved")] + \
               [("specs", C.POINTER(PgRunsSpec))] + \
               [(k, C.c_void_p) for k in ("tables", "run_rows", "group_offsets", "group_runs", "contrast_weights",
                                          "run_table", "group_table", "contrast_table", "status")]


# dxrl_pg_adam_step_ctl: the control struct, the state slots (enum dxrl_pg_opt_slot, with the word
# type of each) and the columns of an iteration's row (enum dxrl_pg_opt_col), in order
class PgLrControl(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("lr_nominal", "lr_min", "lr_max", "target_kl", "stop_factor",
                                          "adapt_factor", "adapt_band")] + \
               [(k, C.c_int32) for k in ("adapt", "pass_index", "last_epoch", "last_pass")] + [("calls", C.c_int64)]


PG_OPT_SLOTS = (("applied", "i64"), ("skipped", "i64"), ("scale", "f64"), ("stopped", "i64"), ("stop_pass", "i64"),
                ("iter_applied", "i64"), ("iter_skipped", "i64"), ("lr_first", "f64"), ("lr_last", "f64"),
                ("kl_max", "f64"), ("kl_sum", "f64"), ("kl_rows", "f64"))
PG_OPT_NAMED = len(PG_OPT_SLOTS)            # DXRL_PG_OPT_NAMED
PG_OPT_SLOT_WORDS = 16                      # DXRL_PG_OPT_SLOT_WORDS
PG_OPT_STATE_WORDS = 2 * PG_OPT_SLOT_WORDS  # DXRL_PG_OPT_STATE_WORDS
PG_OPT_COLUMNS = ("lr", "lr_last", "updates", "skipped", "stop_pass", "kl_max", "kl_epoch", "lr_scale")
PG_OPT_COLS = len(PG_OPT_COLUMNS)           # DXRL_PG_OPT_COLS
PG_KL_RECORD_WORDS = 2                      # DXRL_PG_KL_RECORD_WORDS: a rank's (kl_sum, rows) of a pass


# dxrl_pg_gae_vnorm: the args struct and the words of the state block (enum dxrl_pg_vnorm_word)
class PgGaeVnormArgs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rew", "done", "ep_code", "values")] + \
               [("num_envs", C.c_int64), ("horizon", C.c_int64)] + \
               [(k, C.c_double) for k in ("gamma", "lam", "eps")] + \
               [(k, C.c_void_p) for k in ("adv", "ret", "ret_norm", "values_raw", "partial", "stats", "counts",
                                          "vnorm")] + \
               [("fold", C.c_int32)]


PG_VNORM_NAMES = ("count", "mean", "m2", "mu", "sigma", "batch_count", "batch_mean", "batch_m2", "adv_count",
                  "adv_mean", "adv_m2", "calls", "eps", "forget")
PG_VNORM_NAMED = len(PG_VNORM_NAMES)  # DXRL_PG_VNORM_NAMED
PG_VNORM_WORDS = 16                   # DXRL_PG_VNORM_WORDS
PG_VNORM = {k: i for i, k in enumerate(PG_VNORM_NAMES)}


# dxrl_pg_popart_rescale: the args struct, the words of its state block (enum dxrl_pg_popart_word)
# and the columns of the row it writes (enum dxrl_pg_vnorm_log_col)
class PgPopartArgs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("params", "packed", "vnorm", "popart", "row_out")]


PG_POPART_NAMES = ("mu_head", "sigma_head", "rescales", "skipped", "last_scale", "last_shift")
PG_POPART_NAMED = len(PG_POPART_NAMES)  # DXRL_PG_POPART_NAMED
PG_POPART_WORDS = 8                     # DXRL_PG_POPART_WORDS
PG_POPART = {k: i for i, k in enumerate(PG_POPART_NAMES)}
PG_VNORM_LOG_COLUMNS = ("mu", "sigma", "mu_prev", "sigma_prev", "scale", "shift", "rescaled", "count", "mean", "std",
                        "batch_mean", "batch_std", "calls", "forget")
PG_VNORM_LOG_COLS = len(PG_VNORM_LOG_COLUMNS)  # DXRL_PG_VNORM_LOG_COLS


# the structs added after tests/test_native_abi.py fixed its list: (C name, mirror), sized against
# include/dxrl.h by the tests of the layers that use them
LATER_STRUCTS = (("dxrl_pg_log_args", PgLogArgs), ("dxrl_pg_log_header", PgLogHeader),
                 ("dxrl_pg_val_args", PgValArgs), ("dxrl_pg_val_header", PgValHeader),
                 ("dxrl_pg_val_levels_args", PgValLevelsArgs), ("dxrl_pg_val_paired_args", PgValPairedArgs),
                 ("dxrl_pg_val_failure_args", PgValFailureArgs), ("dxrl_pg_runs_spec", PgRunsSpec),
                 ("dxrl_pg_runs_args", PgRunsArgs), ("dxrl_pg_gae_vnorm_args", PgGaeVnormArgs),
                 ("dxrl_pg_popart_args", PgPopartArgs))

_P = C.c_void_p
_I32,_I64, _F64 = C.c_int32, C.c_int64, C.c_double
_SIGS = {
    "dxrl_abi_version": (C.c_int, []),
    "dxrl_last_error": (C.c_char_p, []),
    "dxrl_env_layout_for": (C.c_int, [C.POINTER(EnvConfig), C.POINTER(EnvLayout)]),
    "dxrl_env_create": (C.c_int, [C.POINTER(EnvConfig), C.c_int32, _P, _P, C.POINTER(_P)]),
    "dxrl_env_destroy": (C.c_int, [_P]),
    "dxrl_env_set_curricula": (C.c_int, [_P, C.POINTER(Curriculum), C.c_int32, _P, _P]),
    "dxrl_env_set_curricula_async": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "dxrl_env_reset": (C.c_int, [_P, _P, _P, _P, _P]),
    "dxrl_env_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "dxrl_env_observe": (C.c_int, [_P, _P, _P]),
    "dxrl_reward_compute": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                      _P, _P, _P]),
    "dxrl_env_set_max_episode_steps": (C.c_int, [_P, C.c_int32]),
    "dxrl_learner_layout_for": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(LearnerLayout)]),
    "dxrl_learner_init": (C.c_int, [C.c_int32, C.c_int32, _P, _P]),
    "dxrl_learner_reset": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P]),
    "dxrl_learner_select": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_double, _P, _P, _P]),
    "dxrl_learner_update": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_double, C.c_double, _P, _P, _P, _P]),
    "dxrl_rollout_simple": (C.c_int, [_P, _P, C.POINTER(LearnerConfig), C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(RolloutIO), _P]),
    "dxrl_study_layout_for": (C.c_int, [C.c_int32, C.POINTER(StudyLayout)]),
    "dxrl_study_init": (C.c_int, [C.c_int32, C.c_int32, _P, _P]),
    "dxrl_study_set_groups": (C.c_int, [_P, C.POINTER(StudyGroup), C.c_int32, _P, _P]),
    "dxrl_rollout_curriculum": (C.c_int, [_P, _P, C.POINTER(LearnerConfig), C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(RolloutIO), C.POINTER(StudyArgs), _P]),
    "dxrl_gemm_bf16": (C.c_int, [_I32, _P, _I64, _P, _I64, _I64, _I32, _I32, _P, _I64, _I32, _P, _I64, _P, _I64,
                                 _P, _I64, _P, _I64, _P, _I64, _I32, _P, _P]),
    "dxrl_wgrad_bf16": (C.c_int, [_I32, _P, _I64, _I32, _P, _I64, _I32, _I64, _I32, _P, _P, _P]),
    "dxrl_pg_sizes": (C.c_int, [C.POINTER(_I64), C.POINTER(_I64)]),
    "dxrl_pg_pack_weights": (C.c_int, [_I32, _P, _P, _P]),
    "dxrl_pg_rollout": (C.c_int, [_P, _P, _P, C.POINTER(PgRolloutArgs), _P]),
    "dxrl_pg_gae": (C.c_int, [_I32, _P, _P, _P, _I64, _I64, _F64, _F64, _P, _P, _P, _P, _P]),
    "dxrl_pg_gae_partial_doubles": (C.c_int, [_I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_gae_timelimit": (C.c_int, [_I32, _P, _P, _P, _I64, _I64, _F64, _F64, _P, _P, _P, _P, _P, _P]),
    "dxrl_pg_gae_timelimit_count_words": (C.c_int, [_I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_gae_vnorm": (C.c_int, [_I32, C.POINTER(PgGaeVnormArgs), _P]),
    "dxrl_pg_gae_vnorm_partial_doubles": (C.c_int, [_I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_vnorm_combine": (C.c_int, [_I32, _P, _I32, _P, _P, _P]),
    "dxrl_pg_popart_rescale": (C.c_int, [_I32, C.POINTER(PgPopartArgs), _P]),
    "dxrl_pg_adv_finalize": (C.c_int, [_I32, _I32, _P, _I64, _P, _P, _P]),
    "dxrl_pg_adv_combine": (C.c_int, [_I32, _P, _I32, _P, _P]),
    "dxrl_pg_heads": (C.c_int, [_I32, C.POINTER(PgHeadsArgs), _P]),
    "dxrl_pg_grad_sumsq": (C.c_int, [_I32, _P, _I64, _P, _P, _P]),
    "dxrl_pg_fused_sizes": (C.c_int, [C.POINTER(_I32), C.POINTER(_I64)]),
    "dxrl_pg_fused": (C.c_int, [_I32, C.POINTER(PgFusedArgs), _P]),
    "dxrl_pg_fused_pair": (C.c_int, [_I32, C.POINTER(PgFusedArgs), C.POINTER(PgFusedArgs), _P]),
    "dxrl_pg_fused_pair_gnorm": (C.c_int, [_I32, C.POINTER(PgFusedArgs), C.POINTER(PgFusedArgs), _P, _I32,
                                           C.POINTER(_I32), _P]),
    "dxrl_pg_rollout_kernel": (C.c_int, [C.c_void_p, _I32, C.POINTER(_I32)]),
    "dxrl_pg_gnorm_blocks": (C.c_int, [C.POINTER(_I32)]),
    "dxrl_evaluate": (C.c_int, [_P, C.POINTER(EvalArgs), _P]),
    "dxrl_evaluate_mlp": (C.c_int, [_P, C.POINTER(EvalArgs), C.POINTER(EvalMlp), _P]),
    "dxrl_eval_summarize": (C.c_int, [_I32, C.POINTER(EvalSummaryArgs), _P]),
    "dxrl_failure_summarize": (C.c_int, [_I32, C.POINTER(FailureSummaryArgs), _P]),
    "dxrl_robustness_summarize": (C.c_int, [_I32, C.POINTER(RobustnessSummaryArgs), _P]),
    "dxrl_study_summarize": (C.c_int, [_I32, C.POINTER(StudySummaryArgs), _P]),
    "dxrl_pg_log_partial_doubles": (C.c_int, [_I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_log_row": (C.c_int, [_I32, C.POINTER(PgLogArgs), _P]),
    "dxrl_pg_log_rank_pack": (C.c_int, [_I32, C.POINTER(PgLogArgs), _P, _P]),
    "dxrl_pg_log_row_world": (C.c_int, [_I32, C.POINTER(PgLogArgs), _P, _I32, _P, _P]),
    "dxrl_pg_val_partial_doubles": (C.c_int, [_I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_val_row": (C.c_int, [_I32, C.POINTER(PgValArgs), _P]),
    "dxrl_pg_val_levels_partial_doubles": (C.c_int, [_I32, _I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_val_levels_row": (C.c_int, [_I32, C.POINTER(PgValLevelsArgs), _P]),
    "dxrl_pg_val_paired_partial_doubles": (C.c_int, [_I32, _I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_val_paired_row": (C.c_int, [_I32, C.POINTER(PgValPairedArgs), _P]),
    "dxrl_pg_val_failure_partial_doubles": (C.c_int, [_I32, _I64, _I64, C.POINTER(_I64)]),
    "dxrl_pg_val_failure_row": (C.c_int, [_I32, C.POINTER(PgValFailureArgs), _P]),
    "dxrl_pg_runs_summarize": (C.c_int, [_I32, C.POINTER(PgRunsArgs), _P]),
    "dxrl_sched_scratch_bytes": (C.c_int, [_I32, _I32, _I64, _I32, C.POINTER(_I64)]),
    "dxrl_sched_scan": (C.c_int, [_I32, C.POINTER(SchedArgs), _P]),
    "dxrl_sched_pack_words": (C.c_int, [_I32, _I64, _I32, _I32, C.POINTER(_I64)]),
    "dxrl_sched_pack": (C.c_int, [_I32, _P, _I32, _I64, _I32, _I32, _P, _P]),
    "dxrl_sched_packed_scratch_bytes": (C.c_int, [_I32, _I32, _I64, _I32, C.POINTER(_I64)]),
    "dxrl_sched_scan_packed": (C.c_int, [_I32, C.POINTER(SchedPackedArgs), _P]),
    "dxrl_sched_candidate_steps": (C.c_int, [_I32, _P, _I32, _I64, _I32, _I32, _P, _P, _P, _P]),
    "dxrl_sched_finish": (C.c_int, [_I32, _P, _P, _P]),
    "dxrl_pg_adam": (C.c_int, [_I32, _P, _P, _P, _P, _I64, _F64, _F64, _F64, _F64, _I64, _P, _F64, _P]),
    "dxrl_pg_optimizer_step": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P, _I64, _F64, _F64, _F64, _F64, _I64, _F64,
                                         _P, _P, _P, _P]),
    "dxrl_pg_adam_step": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P, _I64, _F64, _F64, _F64, _F64, _I64, _F64, _P,
                                    _I32, _P, _P, _P]),
    "dxrl_pg_adam_step_ctl": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P, _I64, _F64, _F64, _F64, _F64, _P, _I32, _P,
                                        _P, _P, _I32, _I64, PgLrControl, _P, _P, _P]),
    "dxrl_pg_kl_rank_pack": (C.c_int, [_I32, _P, _I32, _I64, _P, _P]),
    "dxrl_pg_adam_step_ctl_world": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P, _I64, _F64, _F64, _F64, _F64, _P, _I32,
                                              _P, _P, _P, _I32, PgLrControl, _P, _P, _P]),
}

_lib = None
_lock = threading.Lock()


class NativeError(RuntimeError):
    pass


def lib():
    """Load libdxrl.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NativeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                                  "(there is no CPU fallback)")
            h = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(h, name)
                fn.restype = res
                fn.argtypes = args
            if h.dxrl_abi_version() != ABI_VERSION:
                raise NativeError("libdxrl.so ABI version mismatch; rebuild")
            _lib = h
    return _lib


def check(rc: int, what: str = ""):
    if rc == DXRL_OK:
        return
    msg = lib().dxrl_last_error().decode(errors="replace")
    if rc in (DXRL_E_INVALID, DXRL_E_UNSUPPORTED):
        raise ValueError(f"{what}: {msg}")
    raise NativeError(f"{what}: {msg} (status {rc})")


def call(name: str, *args):
    check(getattr(lib(), name)(*args), name)


def gae_partial_doubles(num_envs: int, horizon: int) -> int:
    """f64 elements of dxrl_pg_gae's `partial` scratch (include/dxrl.h)."""
    out = C.c_int64()
    call("dxrl_pg_gae_partial_doubles", num_envs, horizon, C.byref(out))
    return out.value


def gae_timelimit_count_words(num_envs: int, horizon: int) -> int:
    """i64 elements of dxrl_pg_gae_timelimit's `counts` (include/dxrl.h)."""
    out = C.c_int64()
    call("dxrl_pg_gae_timelimit_count_words", num_envs, horizon, C.byref(out))
    return out.value


def gae_vnorm_partial_doubles(num_envs: int, horizon: int) -> int:
    """f64 elements of dxrl_pg_gae_vnorm's `partial` scratch (include/dxrl.h)."""
    out = C.c_int64()
    call("dxrl_pg_gae_vnorm_partial_doubles", num_envs, horizon, C.byref(out))
    return out.value


def vnorm_fresh(device=None):
    """A fresh dxrl_pg_gae_vnorm state block: f64 [PG_VNORM_WORDS], all zero but sigma = 1."""
    import torch
    t = torch.zeros(PG_VNORM_WORDS, dtype=torch.float64)
    t[PG_VNORM["sigma"]] = 1.0
    return t if device is None else t.to(device)


def popart_fresh(device=None):
    """A fresh dxrl_pg_popart_rescale state block: f64 [PG_POPART_WORDS], all zero but sigma_head = 1."""
    import torch
    t = torch.zeros(PG_POPART_WORDS, dtype=torch.float64)
    t[PG_POPART["sigma_head"]] = 1.0
    return t if device is None else t.to(device)


def ptr(t) -> int | None:
    """Device address of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_of(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise NativeError("no HIP device visible: the dxrl hot path runs only on the GPU (no CPU fallback)")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError(f"device must be a GPU device, got {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def aligned_empty(nbytes: int, device, align: int = 256):
    """uint8 device buffer whose data_ptr is `align`-aligned; returns (owner, view)."""
    owner = torch.empty(nbytes + align, dtype=torch.uint8, device=device)
    off = (-owner.data_ptr()) % align
    return owner, owner[off:off + nbytes]
