"""Curriculum-ablation drivers -- evaluation/curriculum_ablation.py:25-357 -- on the fused
SimpleLearner rollout with a per-lane scheduler (``dxrl_rollout_curriculum``).

One lane is one training run: one env instance (sticky object), one SimpleLearner and one
curriculum scheduler.  The scheduler sits where the lane's episodes end, inside the rollout
kernel, so a run whose difficulty changes between two of its own episodes needs no host round
trip, and a whole study -- thousands of independent runs, both arms -- is one launch.

The device runs the progression rule in integers only.  The host reduces a scheduler prototype
to what the kernel needs:

* the LEVEL TABLE: a real ``CurriculumScheduler`` / ``StepBasedScheduler`` is stepped through
  ``_progress()`` until it stops, collecting the difficulty level and ``get_current_config()``
  of every level (ten steps of 0.1 take eleven progressions to reach 1.0); the configs become
  rows of the env's curriculum table;
* ``min_successes``: the smallest count c with ``c / window >= threshold`` in f64, which is what
  ``np.mean(window of bools) >= threshold`` (curriculum_scheduler.py:182-186) tests.

After the run each lane's ``(success, steps)`` records are replayed through a fresh host
scheduler (``update_batch``); the replay yields ``scheduler_stats`` and must reproduce the
device's level sequence (``RuntimeError`` otherwise).

Parity mode (default) replays the reference's RNG streams per lane (training.ReferenceStreams)
in chunks of ``chunk_steps``; throughput mode (``device_streams=True``) draws from per-run Philox
streams and runs the whole study in one launch.

Quirk kept: ``run_episode`` reports ``success = info.get("success", False) = False``
(episode_utils.py:52), so with ``success_rule="training"`` (the default, the reference's
behaviour) a scheduler with a threshold > 0 never moves and every success rate is 0.
``success_rule="terminated"`` (success = the episode terminated, evaluator.py:157) is this
build's meaningful variant.

Device summary (``summarize_runs``, ``run_ablation_study(device_summary=True)``): the whole study
is one launch whose episode records stay on the device; ``dxrl_study_summarize`` reduces them to
one row per run (the lane table) and one row per arm (the group tables), and only those reach the
host.  ``aggregate_metrics`` also reports medians: they are taken on the host from the lane table
-- 96 bytes per run against ``record_cap`` x 21 bytes of episode records -- which is deliberate;
both modes report the bytes they copy (``BYTES_COPIED``).  The host scheduler replay is not run
in this mode.
"""
from __future__ import annotations

import copy
import ctypes as C
import json
import os
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .experiments import CurriculumConfig, CurriculumScheduler, StepBasedScheduler

MAX_WINDOW = 64


# ------------------------------------------------------------------ host reduction
def fresh_scheduler(proto: CurriculumScheduler) -> CurriculumScheduler:
    """An independent copy of ``proto`` in its initial state (curriculum_scheduler.py:265-273)."""
    s = copy.deepcopy(proto)
    s.reset()
    if isinstance(s, StepBasedScheduler):
        s.current_milestone_idx = 0
    return s


def level_table(proto: CurriculumScheduler) -> Tuple[List[float], List[CurriculumConfig]]:
    """(difficulty level, config) of level 0 and of every level ``_progress()`` reaches.
    ``len(levels) - 1`` is the number of progressions that raise the level."""
    s = fresh_scheduler(proto)
    levels, configs = [s.get_difficulty_level()], [s.get_current_config()]
    while s._progress(rate=0.0):  # the rate only feeds the history entry
        levels.append(s.get_difficulty_level())
        configs.append(s.get_current_config())
        if len(levels) > N.MAX_CURRICULA:
            raise ValueError(f"a scheduler with more than {N.MAX_CURRICULA} levels does not fit the curriculum table")
    return levels, configs


def min_successes(window: int, threshold: float) -> int:
    """Smallest c in 0..window with ``np.mean(c Trues among window bools) >= threshold``;
    0 when threshold <= 0, window + 1 when no count reaches it."""
    w = np.float64(window)
    for c in range(int(window) + 1):
        if np.float64(c) / w >= threshold:  # np.mean of bools: the exact f64 sum c, divided by the count
            return c
    return int(window) + 1


class _Arm:
    def __init__(self, proto: Any):
        self.proto = proto
        self.first_row = 0
        if isinstance(proto, CurriculumScheduler):
            step = isinstance(proto, StepBasedScheduler)
            t = type(proto)
            own = ((t.update is CurriculumScheduler.update and t._should_progress is StepBasedScheduler._should_progress
                    and t._progress is StepBasedScheduler._progress) if step else proto._uses_success_window_rule())
            if not own:
                raise ValueError("the device restates CurriculumScheduler's success-window rule and "
                                 "StepBasedScheduler's milestone rule only")
            self.mode = N.STUDY_STEP_MILESTONES if step else N.STUDY_SUCCESS_WINDOW
            if not step and proto.window_size > MAX_WINDOW:
                raise ValueError(f"window_size {proto.window_size} > {MAX_WINDOW}: the device keeps the success "
                                 "window as a 64-bit mask")
            if step and len(proto.step_milestones) > N.STUDY_MAX_MILESTONES:
                raise ValueError(f"at most {N.STUDY_MAX_MILESTONES} step milestones")
            self.levels, self.configs = level_table(proto)
            if step and len(self.levels) - 1 != len(proto.step_milestones):
                raise ValueError("StepBasedScheduler: one level per milestone expected")
        else:
            if not hasattr(proto, "get_object_size"):
                raise TypeError("an arm is a CurriculumConfig, a CurriculumScheduler or a StepBasedScheduler")
            self.mode = N.STUDY_FIXED
            self.levels, self.configs = [None], [proto]

    @property
    def num_levels(self) -> int:
        return len(self.levels) - 1

    def group(self) -> "N.StudyGroup":
        g = N.StudyGroup()
        g.mode, g.first_row, g.num_levels = self.mode, self.first_row, self.num_levels
        p = self.proto
        if self.mode == N.STUDY_SUCCESS_WINDOW:
            g.window = int(p.window_size)
            g.min_successes = min_successes(p.window_size, p.success_rate_threshold)
            g.min_episodes = int(p.min_episodes_before_progression)
        elif self.mode == N.STUDY_STEP_MILESTONES:
            g.num_milestones = len(p.step_milestones)
            for k, m in enumerate(p.step_milestones):
                g.milestones[k] = int(m)
        return g

    def check_parity_rows(self):
        """The reset tape is resolved on the host before the launch, so every level of the arm
        must consume the same draw slots from the same ranges."""
        def key(c):
            return (c.object_size_range, c.object_mass_range, c.friction_range)
        if any(key(c) != key(self.configs[0]) for c in self.configs[1:]):
            raise ValueError("parity mode resolves the reset draws on the host: the levels of a scheduler arm must "
                             "share their size / mass / friction ranges (use device_streams=True otherwise)")


class StudyPlan:
    """Arms (fixed configs and scheduler prototypes) -> one curriculum table + the lane groups."""

    def __init__(self, arms: Sequence[Any]):
        if not 1 <= len(arms) <= N.STUDY_MAX_GROUPS:
            raise ValueError(f"a study has 1..{N.STUDY_MAX_GROUPS} arms per launch")
        self.arms = [_Arm(a) for a in arms]
        self.table: List[CurriculumConfig] = []
        for a in self.arms:
            a.first_row = len(self.table)
            self.table += a.configs
        if len(self.table) > N.MAX_CURRICULA:
            raise ValueError(f"the arms' levels need {len(self.table)} curriculum rows; the table holds "
                             f"{N.MAX_CURRICULA}")
        self.groups = (N.StudyGroup * len(self.arms))(*[a.group() for a in self.arms])


def replay_scheduler(arm: _Arm, success, steps, ep_level) -> Dict:
    """Feed the lane's records to a fresh host scheduler; its progression points must be the
    device's.  Returns the scheduler's statistics (curriculum_scheduler.py:242-263)."""
    s = fresh_scheduler(arm.proto)
    s.update_batch(np.asarray(success, dtype=bool), np.asarray(steps, dtype=np.int64))
    seq = np.zeros(len(steps), dtype=np.int64)
    for h in s.progression_history:
        seq[h["episode"] - 1:] += 1
    if not np.array_equal(seq, np.asarray(ep_level, dtype=np.int64)):
        raise RuntimeError("the device's curriculum levels differ from the host scheduler's replay: "
                           f"device {np.asarray(ep_level).tolist()} host {seq.tolist()}")
    return s.get_statistics()


# ------------------------------------------------------------------ device study
class DeviceStudy:
    """Env + learners + schedulers of ``len(lane_arm)`` runs on one device."""

    def __init__(self, plan: StudyPlan, lane_arm: Sequence[int], max_episode_steps: int = 200,
                 learning_rate: float = 0.01, reward_type: str = "dense", success_rule: str = "training",
                 device=None, env_seed: int = 0, learner_seed: int = 0, lane_stream: Optional[Sequence[int]] = None):
        from .envs import VecEnv
        from .policies import VecSimpleLearner
        if success_rule not in ("training", "terminated"):
            raise ValueError("success_rule must be 'training' (episode_utils.py:52) or 'terminated' "
                             "(evaluator.py:157)")
        self.plan = plan
        self.lane_arm = np.asarray(lane_arm, dtype=np.int32)
        n = self.n = len(self.lane_arm)
        if n == 0 or self.lane_arm.min() < 0 or self.lane_arm.max() >= len(plan.arms):
            raise ValueError("every lane names one of the plan's arms")
        self.max_steps = int(max_episode_steps)
        self.success_rule = N.SUCCESS_TRAINING if success_rule == "training" else N.SUCCESS_TERMINATED
        self.env = VecEnv(n, reward_type=reward_type, max_episode_steps=max_episode_steps, seed=env_seed,
                          device=device)
        dev = self.device = self.env.device
        self.rows = np.array([plan.arms[a].first_row for a in self.lane_arm], dtype=np.int32)
        self.env.set_curricula(plan.table, env_index=self.rows)
        self.learner = VecSimpleLearner(n, learning_rate=learning_rate, seed=learner_seed, device=dev)
        self._lcfg = self.learner.native_config()
        lay = N.StudyLayout()
        N.call("dxrl_study_layout_for", n, C.byref(lay))
        self.layout = lay
        self._owner, self.state = N.aligned_empty(lay.total_bytes, dev)
        self._gowner, self.groups_dev = N.aligned_empty(C.sizeof(N.StudyGroup) * len(plan.arms), dev)
        with torch.cuda.device(dev):
            N.call("dxrl_study_set_groups", self.env.handle, plan.groups, len(plan.arms), N.ptr(self.groups_dev),
                   self.env._stream())
        self.lane_group = torch.from_numpy(self.lane_arm).to(dev)
        self.lane_stream = (None if lane_stream is None
                            else torch.from_numpy(np.asarray(lane_stream, dtype=np.int64)).to(dev))
        self.ep_count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.gauss_used = torch.zeros(n, dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.record_cap = 0
        self.init()

    def init(self):
        """Fresh learners and schedulers (the env is reset by ``start``)."""
        self.learner.init()
        N.call("dxrl_study_init", self.device.index, self.n, N.ptr(self.state), self.env._stream())

    def _view(self, off, dtype):
        nbytes = self.n * torch.empty((), dtype=dtype).element_size()
        return self.state[off:off + nbytes].view(dtype)

    @property
    def level(self) -> torch.Tensor:
        return self._view(self.layout.level, torch.int32)

    @property
    def total_episodes(self) -> torch.Tensor:
        return self._view(self.layout.total_episodes, torch.int32)

    @property
    def total_steps(self) -> torch.Tensor:
        return self._view(self.layout.total_steps, torch.int64)

    @property
    def window_mask(self) -> torch.Tensor:
        """The success windows (u64, newest episode in bit 0) as int64."""
        return self._view(self.layout.window_mask, torch.int64)

    @property
    def milestone(self) -> torch.Tensor:
        return self._view(self.layout.milestone, torch.int32)

    def reserve(self, record_cap: int):
        if record_cap > self.record_cap:
            n, dev = self.n, self.device
            self.record_cap = int(record_cap)
            self.ep_return = torch.empty(n, record_cap, dtype=torch.float64, device=dev)
            self.ep_length = torch.empty(n, record_cap, dtype=torch.int32, device=dev)
            self.ep_success = torch.empty(n, record_cap, dtype=torch.uint8, device=dev)
            self.ep_end = torch.empty(n, record_cap, dtype=torch.int32, device=dev)
            self.ep_level = torch.empty(n, record_cap, dtype=torch.int32, device=dev)

    def start(self, draws: torch.Tensor):
        """Episode 0 of every run: env.reset() + policy.reset() (episode_utils.py:33-36)."""
        self.env.reset(draws=draws, write_obs=False)
        self.learner.reset()

    def launch(self, num_steps: int, episode_budget: Optional[torch.Tensor] = None,
               gauss: Optional[torch.Tensor] = None, resets: Optional[torch.Tensor] = None):
        """One ``dxrl_rollout_curriculum`` call on the current stream (no host sync)."""
        io = N.RolloutIO()
        io.record_cap = self.record_cap
        if self.record_cap:
            io.ep_return, io.ep_length = N.ptr(self.ep_return), N.ptr(self.ep_length)
            io.ep_success, io.ep_end_step = N.ptr(self.ep_success), N.ptr(self.ep_end)
        io.ep_count, io.gauss_used, io.status = N.ptr(self.ep_count), N.ptr(self.gauss_used), N.ptr(self.status)
        io.episode_budget = N.ptr(episode_budget)
        if gauss is not None:
            io.gauss, io.gauss_stride = N.ptr(gauss), gauss.shape[1]
            io.reset_draws, io.reset_stride = N.ptr(resets), resets.shape[1]
        st = N.StudyArgs()
        st.groups, st.num_groups = N.ptr(self.groups_dev), len(self.plan.arms)
        st.lane_group, st.sched_state = N.ptr(self.lane_group), N.ptr(self.state)
        st.ep_level = N.ptr(self.ep_level) if self.record_cap else None
        st.lane_stream = N.ptr(self.lane_stream)
        self.status.zero_()
        N.call("dxrl_rollout_curriculum", self.env.handle, N.ptr(self.learner.state), C.byref(self._lcfg),
               int(num_steps), self.max_steps, self.success_rule, C.byref(io), C.byref(st), self.env._stream())

    def check_status(self):
        s = int(self.status.item())
        if s & 1:
            raise N.NativeError("parity tape overrun in dxrl_rollout_curriculum")
        if s & 2:
            raise N.NativeError("dxrl_rollout_curriculum: a lane's group or curriculum row lies outside its table")

    def records(self) -> List[Dict[str, np.ndarray]]:
        """This call's finished episodes per lane, in completion order."""
        cnt = self.ep_count.cpu().numpy()
        if (cnt > self.record_cap).any():
            raise N.NativeError("episode records dropped: record_cap too small")
        cols = {"reward": self.ep_return, "steps": self.ep_length, "success": self.ep_success,
                "level": self.ep_level, "end_step": self.ep_end}
        host = {k: v.cpu().numpy() for k, v in cols.items()}
        BYTES_COPIED["records"] += cnt.nbytes + sum(v.nbytes for v in host.values())
        return [{k: v[i, :cnt[i]].copy() for k, v in host.items()} for i in range(self.n)]

    def close(self):
        self.env.close()


def _entropy_seed() -> int:
    return int(np.random.SeedSequence().entropy)


def philox_start_draws(study: DeviceStudy, seed: int, lane_stream: Sequence[int]) -> torch.Tensor:
    """Throughput mode's first reset of every run, keyed by (seed, the run's stream id) so that it
    does not depend on the lane a run occupies."""
    from .envs import RESET_SLOTS, resolve_reset_draws
    recs = np.empty((study.n, RESET_SLOTS))
    for i, sid in enumerate(lane_stream):
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & (2**64 - 1), int(sid)])))
        recs[i], *_ = resolve_reset_draws(rng, study.plan.table[int(study.rows[i])], first=True)
    return torch.from_numpy(recs).to(study.device)


def train_runs(jobs: Sequence[Tuple[Any, int]], num_episodes: int, max_episode_steps: int = 200,
               learning_rate: float = 0.01, success_rule: str = "training",
               env_seeds: Optional[Sequence[Optional[int]]] = None, device=None, chunk_steps: int = 2048,
               reward_type: str = "dense", device_streams: bool = False, stream_seed: int = 0) -> List[Dict]:
    """Every (arm, learner seed) job as one lane.  An arm is a fixed ``CurriculumConfig``, a
    ``CurriculumScheduler`` prototype or a ``StepBasedScheduler`` prototype (never mutated); jobs
    naming the same object share a group.  Returns per job ``episode_rewards``, ``episode_steps``,
    ``success_rates``, ``difficulty_levels`` and ``scheduler_stats`` (scheduler arms), plus
    ``gauss_used`` (the learner's np.random draws, parity mode).

    Parity mode: lane k replays ``np.random.seed(jobs[k][1])`` and the gymnasium stream of
    ``env_seeds[k]`` (None = OS entropy, as the reference).  ``device_streams=True``: Philox
    streams keyed by ``stream_seed`` and the job's seed, the whole run in one launch."""
    from .training import ReferenceStreams
    from .envs import ACTION_DIM
    arms: List[Any] = []
    lane_arm = []
    for arm, _ in jobs:
        k = next((j for j, a in enumerate(arms) if a is arm), None)
        if k is None:
            arms.append(arm)
            k = len(arms) - 1
        lane_arm.append(k)
    plan = StudyPlan(arms)
    if not device_streams:
        for a in plan.arms:
            a.check_parity_rows()
    n, E = len(jobs), int(num_episodes)
    seeds = [int(s) for _, s in jobs]
    BYTES_COPIED["records"] = 0
    study = DeviceStudy(plan, lane_arm, max_episode_steps, learning_rate, reward_type, success_rule, device,
                        env_seed=stream_seed, learner_seed=stream_seed + 1,
                        lane_stream=seeds if device_streams else None)
    got: List[List[Dict[str, np.ndarray]]] = [[] for _ in range(n)]
    used = np.zeros(n, dtype=np.int64)
    try:
        if device_streams:
            study.reserve(E)
            study.start(philox_start_draws(study, stream_seed, seeds))
            budget = torch.full((n,), E, dtype=torch.int32, device=study.device)
            study.launch(E * int(max_episode_steps), episode_budget=budget)
            study.check_status()
            for i, r in enumerate(study.records()):
                got[i].append(r)
        else:
            es = list(env_seeds) if env_seeds is not None else [None] * n
            es = [_entropy_seed() if s is None else int(s) for s in es]
            streams = ReferenceStreams(study.env, es, seeds)
            study.reserve(min(int(chunk_steps), E))
            study.start(streams.initial_draws(study.rows))
            remaining = np.full(n, E, dtype=np.int32)
            while remaining.max() > 0:
                gt = streams.gauss_tape(2 * ACTION_DIM * int(chunk_steps))
                rt, states = streams.reset_tape(min(int(chunk_steps), int(remaining.max())), study.rows)
                study.launch(int(chunk_steps), episode_budget=torch.from_numpy(remaining).to(study.device), gauss=gt,
                             resets=rt)
                cnt = study.ep_count.cpu().numpy()
                gu = study.gauss_used.cpu().numpy()
                streams.consume_gauss(gu)
                streams.rewind(states, cnt)
                study.check_status()
                used += gu
                for i, r in enumerate(study.records()):
                    got[i].append(r)
                remaining = np.maximum(remaining - cnt.astype(np.int32), 0)
    finally:
        study.close()
    out = []
    for i in range(n):
        rec = {k: np.concatenate([c[k] for c in got[i]]) for k in ("reward", "steps", "success", "level")}
        arm = plan.arms[lane_arm[i]]
        res = {"episode_rewards": [float(x) for x in rec["reward"]], "episode_steps": [int(x) for x in rec["steps"]],
               "success_rates": [1.0 if s else 0.0 for s in rec["success"]]}
        if arm.mode != N.STUDY_FIXED:
            res["difficulty_levels"] = [float(arm.levels[int(k)]) for k in rec["level"]]
            res["scheduler_stats"] = replay_scheduler(arm, rec["success"], rec["steps"], rec["level"])
        res["gauss_used"] = int(used[i])
        out.append(res)
    return out


# ------------------------------------------------------------------ device summary
BYTES_COPIED = {"records": 0, "summary": 0}  # device -> host bytes of the last study, per mode
SUMMARY_KEYS = ("convergence_episode", "convergence_steps", "reward_variance", "reward_std",
                "coefficient_of_variation", "final_reward", "final_success_rate", "mean_reward",
                "overall_success_rate")
_L_E, _L_STEPS, _L_SUCC, _L_FWS, _L_CONV, _L_RCONV, _L_LEVEL, _L_FLAGS = range(8)


def launch_runs(jobs: Sequence[Tuple[Any, int]], num_episodes: int, max_episode_steps: int = 200,
                learning_rate: float = 0.01, success_rule: str = "training",
                env_seeds: Optional[Sequence[Optional[int]]] = None, device=None, reward_type: str = "dense",
                device_streams: bool = False, stream_seed: int = 0) -> DeviceStudy:
    """``train_runs``' launch without its host tail: every job's whole run in ONE
    ``dxrl_rollout_curriculum`` call on the current stream, the episode records left on the device
    (``study.ep_return`` ..., ``study.ep_count``) for ``summarize_runs``.  No host synchronisation
    after the launch; the caller closes the study.  Parity mode resolves the tapes of the whole
    run up front (2 x 15 x num_episodes x max_episode_steps gauss values per lane)."""
    from .training import ReferenceStreams
    from .envs import ACTION_DIM
    arms: List[Any] = []
    lane_arm = []
    for arm, _ in jobs:
        k = next((j for j, a in enumerate(arms) if a is arm), None)
        if k is None:
            arms.append(arm)
            k = len(arms) - 1
        lane_arm.append(k)
    plan = StudyPlan(arms)
    if not device_streams:
        for a in plan.arms:
            a.check_parity_rows()
    n, E = len(jobs), int(num_episodes)
    steps = E * int(max_episode_steps)
    seeds = [int(s) for _, s in jobs]
    study = DeviceStudy(plan, lane_arm, max_episode_steps, learning_rate, reward_type, success_rule, device,
                        env_seed=stream_seed, learner_seed=stream_seed + 1,
                        lane_stream=seeds if device_streams else None)
    try:
        study.reserve(E)
        budget = torch.full((n,), E, dtype=torch.int32, device=study.device)
        if device_streams:
            study.start(philox_start_draws(study, stream_seed, seeds))
            study.launch(steps, episode_budget=budget)
        else:
            es = list(env_seeds) if env_seeds is not None else [None] * n
            es = [_entropy_seed() if s is None else int(s) for s in es]
            streams = ReferenceStreams(study.env, es, seeds)
            study.start(streams.initial_draws(study.rows))
            gt = streams.gauss_tape(2 * ACTION_DIM * steps)
            rt, _ = streams.reset_tape(E, study.rows)
            study.launch(steps, episode_budget=budget, gauss=gt, resets=rt)
            study._tapes = (gt, rt)  # alive until the launch has run
    except Exception:
        study.close()
        raise
    study.num_episodes = E
    return study


def _int_moments(n: int, s1: int, s2: int, scale: float) -> Tuple[float, float]:
    """(mean, population std) of n integers with sum s1 and sum of squares s2, each divided by
    ``scale``: the variance numerator n s2 - s1^2 is an exact integer."""
    return s1 / (n * scale), float(np.sqrt(float(max(n * s2 - s1 * s1, 0)))) / (n * scale)


def lane_metrics_row(ints: np.ndarray, reals: np.ndarray, window: int) -> Dict:
    """One lane-table row as ``compute_convergence_metrics``' dictionary."""
    E = int(ints[_L_E])
    conv = None if ints[_L_RCONV] < 0 else int(ints[_L_RCONV])
    var = reals[2] / reals[0]
    std, mean = np.sqrt(var), reals[1]
    with np.errstate(divide="ignore"):
        cv = std / mean if mean != 0 else np.inf
    return {
        "convergence_episode": conv,
        "convergence_steps": float(conv * mean) if conv else None,
        "reward_variance": float(var),
        "reward_std": float(std),
        "coefficient_of_variation": float(cv),
        "final_reward": float(reals[3]),
        "final_success_rate": float(int(ints[_L_FWS]) / min(window, E)),
        "mean_reward": float(mean),
        "overall_success_rate": float(int(ints[_L_SUCC]) / E),
    }


def _statistics_from_lanes(ints: np.ndarray, window: int) -> Dict:
    """``compute_ablation_statistics``' entry of one group from its lane rows (the fall-back for a
    group whose lanes do not share one episode count)."""
    fsr = [int(r[_L_FWS]) / min(window, int(r[_L_E])) for r in ints]
    mel = [int(r[_L_STEPS]) / int(r[_L_E]) for r in ints]
    conv = [int(r[_L_CONV]) for r in ints if r[_L_CONV] >= 0]
    return {"final_success_rate": {"mean": float(np.mean(fsr)), "std": float(np.std(fsr)), "min": float(np.min(fsr)),
                                   "max": float(np.max(fsr))},
            "mean_episode_length": {"mean": float(np.mean(mel)), "std": float(np.std(mel))},
            "convergence_step": {"mean": float(np.mean(conv)) if conv else None,
                                 "std": float(np.std(conv)) if conv else None, "num_converged": len(conv)}}


def group_statistics(stats: np.ndarray, ints: np.ndarray, window: int) -> Dict:
    """``compute_ablation_statistics``' entry of one group from its ``group_stats`` row (``ints``:
    the group's lane rows, read only to see whether they share one episode count)."""
    n = int(stats[0])
    live = ints[ints[:, _L_E] > 0] if len(ints) else ints
    if n == 0:
        raise ValueError("a group without lanes has no statistics")
    if len(set(live[:, _L_E].tolist())) != 1:
        return _statistics_from_lanes(live, window)
    E = int(live[0, _L_E])
    d = min(window, E)
    s = [int(x) for x in stats]
    fm, fs = _int_moments(n, s[4], s[5], d)
    lm, ls = _int_moments(n, s[2], s[3], E)
    k = s[8]
    cm, cs = _int_moments(k, s[9], s[10], 1) if k else (None, None)
    return {"final_success_rate": {"mean": fm, "std": fs, "min": s[6] / d, "max": s[7] / d},
            "mean_episode_length": {"mean": lm, "std": ls},
            "convergence_step": {"mean": cm, "std": cs, "num_converged": k}}


def group_aggregate(stats: np.ndarray, metrics: np.ndarray, ints: np.ndarray, reals: np.ndarray, window: int) -> Dict:
    """``aggregate_metrics``' dictionary of one group: means and stds from the group tables, medians
    (and the two columns the tables do not carry, convergence_steps and overall_success_rate) from
    the group's lane rows."""
    live = ints[:, _L_E] > 0
    ints, reals = ints[live], reals[live]
    rows = [lane_metrics_row(i, r, window) for i, r in zip(ints, reals)]
    n = int(stats[0])
    s = [int(x) for x in stats]
    same = len(set(ints[:, _L_E].tolist())) == 1
    out = {}
    with np.errstate(invalid="ignore"):
        for key in SUMMARY_KEYS:
            vals = [m[key] for m in rows if m[key] is not None]
            if not vals:
                out[key] = None
                continue
            if key == "convergence_episode":
                mean, std = _int_moments(s[11], s[12], s[13], 1)
            elif key == "final_success_rate" and same:
                mean, std = _int_moments(n, s[4], s[5], min(window, int(ints[0, _L_E])))
            elif key in ("reward_variance", "reward_std", "coefficient_of_variation", "final_reward", "mean_reward"):
                k = ("reward_variance", "reward_std", "coefficient_of_variation", "final_reward",
                     "mean_reward").index(key)
                cnt, mean, m2 = (float(x) for x in metrics[k])
                if key == "coefficient_of_variation" and cnt != n:  # a lane with an infinite CV
                    mean, std = float(np.mean(vals)), float(np.std(vals))
                else:
                    std = float(np.sqrt(m2 / cnt))
            else:
                mean, std = float(np.mean(vals)), float(np.std(vals))
            out[key] = {"mean": float(mean), "std": float(std), "median": float(np.median(vals))}
    return out


def summarize_runs(study_or_studies, groups, window: int = 20, threshold: float = 0.5, return_runs: bool = False,
                   timing: Optional[Dict] = None) -> Dict:
    """``dxrl_study_summarize`` on the records one or several launched ``DeviceStudy`` objects hold
    (stream-ordered behind their launches, no host synchronisation before the tables are read).
    The studies' lanes are numbered through in the order given.  ``groups``: ``{name: lane
    indices}``; a lane may be in several groups or in none.  A lane's episode count is the study's
    ``ep_count`` (one launch).

    Returns ``statistics`` (``ablation.compute_ablation_statistics``' form per group),
    ``aggregated_metrics`` (``aggregate_metrics``' form per group), ``final_levels`` (level index
    per lane), ``tie_lanes`` (settled with ``compute_convergence_metrics`` on those lanes' returns),
    ``bytes_copied``, the raw tables, and with ``return_runs`` the per-lane
    ``compute_convergence_metrics`` dictionaries (``runs``).  ``timing``: a dict that receives
    ``summary_ms``, the HIP-event time of the summary launches."""
    studies = [study_or_studies] if isinstance(study_or_studies, DeviceStudy) else list(study_or_studies)
    names = list(groups)
    members = [np.asarray(groups[k], dtype=np.int32).reshape(-1) for k in names]
    dev = studies[0].device
    L = sum(st.n for st in studies)
    G = len(names)
    w = int(window)
    offsets = np.zeros(G + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(m) for m in members])
    flat = np.concatenate(members) if members else np.zeros(0, np.int32)
    if len(flat) and (flat.min() < 0 or flat.max() >= L):
        raise ValueError("a group names a lane outside the studies")
    with torch.cuda.device(dev):
        lane_ints = torch.zeros(L, N.STUDY_LANE_INTS, dtype=torch.int64, device=dev)
        lane_reals = torch.zeros(L, N.STUDY_LANE_REALS, dtype=torch.float64, device=dev)
        group_stats = torch.zeros(max(G, 1), 16, dtype=torch.int64, device=dev)
        group_metrics = torch.zeros(max(G, 1), N.STUDY_METRICS, 3, dtype=torch.float64, device=dev)
        tie = torch.zeros(1 + L, dtype=torch.int32, device=dev)  # [0] the count, [1:] the list
        status = torch.zeros(len(studies), dtype=torch.int32, device=dev)
        goff = torch.from_numpy(offsets).to(dev)
        glanes = torch.from_numpy(flat if len(flat) else np.zeros(1, np.int32)).to(dev)
        cur = torch.cuda.current_stream(dev)
        off = 0
        for st in studies:
            done = getattr(st, "launched", None)  # an event recorded on the stream of the study's launch
            if done is not None:
                cur.wait_event(done)
        if timing is not None:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(cur)
        for k, st in enumerate(studies):
            a = N.StudySummaryArgs()
            a.num_lanes, a.record_cap, a.lane_offset, a.total_lanes = st.n, st.record_cap, off, L
            a.window, a.min_count, a.reward_threshold = w, min_successes(w, 0.5), float(threshold)
            a.ep_return, a.ep_length, a.ep_success = N.ptr(st.ep_return), N.ptr(st.ep_length), N.ptr(st.ep_success)
            a.ep_level = N.ptr(st.ep_level)
            a.lane_episodes = N.ptr(st.ep_count)
            a.lane_ints, a.lane_reals, a.status = N.ptr(lane_ints), N.ptr(lane_reals), N.ptr(status[k:])
            if k == len(studies) - 1:
                a.num_groups, a.num_members, a.tie_cap = G, len(flat), L
                a.group_offsets, a.group_lanes = N.ptr(goff), N.ptr(glanes)
                a.group_stats, a.group_metrics = N.ptr(group_stats), N.ptr(group_metrics)
                a.tie_count, a.tie_list = N.ptr(tie), N.ptr(tie[1:])
            N.call("dxrl_study_summarize", dev.index, C.byref(a), cur.cuda_stream)
            off += st.n
        if timing is not None:
            t1.record(cur)
        host = [t.cpu().numpy() for t in (lane_ints, lane_reals, group_stats, group_metrics, tie, status)]
        if timing is not None:
            timing["summary_ms"] = t0.elapsed_time(t1)
    ints, reals, gstats, gmetrics, tie_h, status_h = host
    copied = sum(x.nbytes for x in host)
    for st in studies:
        st.check_status()
        copied += 4
    code = int(np.bitwise_or.reduce(status_h))
    if code & 1:
        raise N.NativeError("dxrl_study_summarize: a group offset or member lies outside its table")
    if code & 4:
        raise N.NativeError("dxrl_study_summarize: a lane finished no episode or more than record_cap")
    tie_lanes = [int(x) for x in tie_h[1:1 + int(tie_h[0])]]
    starts = np.cumsum([0] + [st.n for st in studies])
    fetched = [0]

    def fetch(row: int) -> np.ndarray:
        k = int(np.searchsorted(starts, row, side="right")) - 1
        r = studies[k].ep_return[row - int(starts[k]), :int(ints[row, _L_E])].cpu().numpy()
        fetched[0] += r.nbytes
        return r

    out = form_summary(ints, reals, gstats[:G], gmetrics[:G], tie_lanes, names, members, w, threshold, fetch,
                       return_runs)
    out["status"] = code
    out["bytes_copied"] = BYTES_COPIED["summary"] = copied + fetched[0]
    return out


def form_summary(ints: np.ndarray, reals: np.ndarray, gstats: np.ndarray, gmetrics: np.ndarray,
                 tie_lanes: Sequence[int], names: Sequence[str], members: Sequence[np.ndarray], window: int,
                 threshold: float, fetch_returns, return_runs: bool = False) -> Dict:
    """The host half of ``summarize_runs``: settles the tie lanes (``fetch_returns(row)`` -> that
    lane's returns; ``np.convolve``'s rounding decides their crossing, and the sums of every group
    that holds them follow), then forms the dictionaries from the tables.  ``ints`` and ``gstats``
    are updated in place."""
    w = int(window)
    for row in tie_lanes:
        r = fetch_returns(int(row))
        want = compute_convergence_metrics(list(r), [0.0] * len(r), w, threshold)["convergence_episode"]
        new, old = (-1 if want is None else int(want)), int(ints[row, _L_RCONV])
        ints[row, _L_RCONV] = new
        for g, m in enumerate(members):
            for _ in range(int((np.asarray(m) == row).sum())):
                if old >= 0:
                    gstats[g, 11:14] -= (1, old, old * old)
                if new >= 0:
                    gstats[g, 11:14] += (1, new, new * new)
    out = {"statistics": {}, "aggregated_metrics": {}, "tie_lanes": [int(x) for x in tie_lanes],
           "final_levels": ints[:, _L_LEVEL].tolist(), "lane_ints": ints, "lane_reals": reals,
           "group_stats": gstats, "group_metrics": gmetrics}
    for g, name in enumerate(names):
        gi, gr = ints[np.asarray(members[g], dtype=np.int64)], reals[np.asarray(members[g], dtype=np.int64)]
        out["statistics"][name] = group_statistics(gstats[g], gi, w)
        out["aggregated_metrics"][name] = group_aggregate(gstats[g], gmetrics[g], gi, gr, w)
    if return_runs:
        out["runs"] = [lane_metrics_row(i, r, w) for i, r in zip(ints, reals)]
    return out


# ------------------------------------------------------------------ the reference's drivers
def reference_scheduler() -> CurriculumScheduler:
    """curriculum_ablation.py:38-48."""
    return CurriculumScheduler(initial_config=CurriculumConfig.easy(), target_config=CurriculumConfig.hard(),
                               success_rate_threshold=0.3, window_size=15, min_episodes_before_progression=20,
                               progression_steps=5)


def _leave_np_random(seed: int, res: Dict) -> Dict:
    # np.random where the reference leaves it: seeded with `seed`, advanced by the learner's draws
    used = res.pop("gauss_used")
    np.random.seed(seed)
    np.random.standard_normal(used)
    return res


def train_with_curriculum(num_episodes: int = 200, seed: int = 42, env_seed: Optional[int] = None,
                          success_rule: str = "training", device=None) -> Dict:
    """curriculum_ablation.py:25-83."""
    (res,) = train_runs([(reference_scheduler(), seed)], num_episodes, success_rule=success_rule,
                        env_seeds=[env_seed], device=device)
    return _leave_np_random(seed, res)


def train_without_curriculum(num_episodes: int = 200, seed: int = 42, use_hard: bool = True,
                             env_seed: Optional[int] = None, success_rule: str = "training", device=None) -> Dict:
    """curriculum_ablation.py:86-134."""
    config = CurriculumConfig.hard() if use_hard else CurriculumConfig.easy()
    (res,) = train_runs([(config, seed)], num_episodes, success_rule=success_rule, env_seeds=[env_seed],
                        device=device)
    return _leave_np_random(seed, res)


def compute_convergence_metrics(episode_rewards: List[float], success_rates: List[float], window_size: int = 20,
                                threshold: float = 0.5) -> Dict:
    """curriculum_ablation.py:137-203 (same NumPy calls; a convergence episode of 0 reports
    ``convergence_steps`` None, as there)."""
    r = np.array(episode_rewards)
    s = np.array(success_rates)
    full = len(r) >= window_size
    reward_ma = np.convolve(r, np.ones(window_size) / window_size, mode="valid") if full else r
    conv = None
    for i, v in enumerate(reward_ma):
        if v >= threshold:
            conv = i + window_size - 1
            break
    std = np.std(r)
    mean = np.mean(r)
    return {
        "convergence_episode": conv,
        "convergence_steps": conv * np.mean(r) if conv else None,
        "reward_variance": float(np.var(r)),
        "reward_std": float(std),
        "coefficient_of_variation": float(std / mean if mean != 0 else np.inf),
        "final_reward": float(np.mean(r[-window_size:]) if full else np.mean(r)),
        "final_success_rate": float(np.mean(s[-window_size:]) if len(s) >= window_size else np.mean(s)),
        "mean_reward": float(mean),
        "overall_success_rate": float(np.mean(s)),
    }


def aggregate_metrics(metrics_list: List[Dict]) -> Dict:
    """curriculum_ablation.py:269-282: mean / std / median of every metric over the runs that
    have it (None when no run does)."""
    out = {}
    for key in metrics_list[0].keys():
        vals = [m[key] for m in metrics_list if m[key] is not None]
        out[key] = ({"mean": float(np.mean(vals)), "std": float(np.std(vals)), "median": float(np.median(vals))}
                    if vals else None)
    return out


def compute_improvements(cur: Dict, no_cur: Dict) -> Dict:
    """curriculum_ablation.py:287-302."""
    out = {}
    for key in cur.keys():
        if cur[key] is not None and no_cur[key] is not None:
            a, b = cur[key]["mean"], no_cur[key]["mean"]
            pct = ((a - b) / abs(b)) * 100 if b != 0 else 0.0
            out[key] = {"absolute": float(a - b), "percentage": float(pct)}
    return out


def _pm(agg: Dict, key: str, fmt: str) -> str:
    a = agg[key]
    return "n/a" if a is None else f"{a['mean']:{fmt}} ± {a['std']:{fmt}}"


def run_ablation_study(num_episodes: int = 200, num_runs: int = 5, output_dir: str = "logs",
                       env_seeds: Optional[Sequence[Optional[int]]] = None, success_rule: str = "training",
                       device_streams: bool = False, device=None, device_summary: bool = False) -> Dict:
    """curriculum_ablation.py:206-357: ``num_runs`` runs with the curriculum (seeds 42 + run) and
    ``num_runs`` on the fixed hard config, all 2 x num_runs runs as lanes of one ``train_runs``
    call; same JSON keys in <output_dir>/curriculum_ablation.json and the same report text.
    ``env_seeds``: the with-curriculum runs' env seeds, then the fixed runs' (None = entropy).
    Where the reference would raise on an aggregate that is None (no run converged), the report
    prints ``n/a``.  ``device_summary=True``: one launch, ``summarize_runs`` and host medians
    instead of ``train_runs`` and the per-run host metrics (same dictionary, JSON and text)."""
    bar = "=" * 60
    print(bar)
    print("Curriculum Learning Ablation Study")
    print(bar)
    os.makedirs(output_dir, exist_ok=True)
    sched, hard = reference_scheduler(), CurriculumConfig.hard()
    jobs = [(sched, 42 + r) for r in range(num_runs)] + [(hard, 42 + r) for r in range(num_runs)]
    summary = None
    if device_summary:
        study = launch_runs(jobs, num_episodes, success_rule=success_rule, env_seeds=env_seeds, device=device,
                            device_streams=device_streams)
        try:
            summary = summarize_runs(study, {"with": range(num_runs), "without": range(num_runs, 2 * num_runs)},
                                     return_runs=True)
        finally:
            study.close()
    else:
        runs = train_runs(jobs, num_episodes, success_rule=success_rule, env_seeds=env_seeds, device=device,
                          device_streams=device_streams)
        for r in runs:
            r.pop("gauss_used")
        cur_results, no_cur_results = runs[:num_runs], runs[num_runs:]
    print(f"\nRunning {num_runs} independent runs...")
    print("Training with curriculum...")
    for run in range(num_runs):
        print(f"  Run {run + 1}/{num_runs}...", end="\r")
    print("\nTraining without curriculum (fixed hard)...")
    for run in range(num_runs):
        print(f"  Run {run + 1}/{num_runs}...", end="\r")
    print("\n" + bar)
    print("Computing metrics...")
    print(bar)
    if summary is not None:
        cur_metrics, no_cur_metrics = summary["runs"][:num_runs], summary["runs"][num_runs:]
        cur_agg, no_cur_agg = summary["aggregated_metrics"]["with"], summary["aggregated_metrics"]["without"]
    else:
        cur_metrics = [compute_convergence_metrics(r["episode_rewards"], r["success_rates"]) for r in cur_results]
        no_cur_metrics = [compute_convergence_metrics(r["episode_rewards"], r["success_rates"])
                          for r in no_cur_results]
        cur_agg, no_cur_agg = aggregate_metrics(cur_metrics), aggregate_metrics(no_cur_metrics)
    improvements = compute_improvements(cur_agg, no_cur_agg)
    print("\n" + bar)
    print("Ablation Study Results")
    print(bar)
    for title, agg in (("\nWITH CURRICULUM:", cur_agg), ("\nWITHOUT CURRICULUM (Fixed Hard):", no_cur_agg)):
        print(title)
        print(f"  Convergence episode: {_pm(agg, 'convergence_episode', '.1f')}")
        print(f"  Reward variance: {_pm(agg, 'reward_variance', '.4f')}")
        print(f"  Reward std: {_pm(agg, 'reward_std', '.4f')}")
        print(f"  Coefficient of variation: {_pm(agg, 'coefficient_of_variation', '.4f')}")
        print(f"  Final reward: {_pm(agg, 'final_reward', '.4f')}")
        print(f"  Final success rate: {_pm(agg, 'final_success_rate', '.4f')}")
    print("\nIMPROVEMENTS (Curriculum vs No Curriculum):")
    for key, imp in improvements.items():
        print(f"  {key}:")
        print(f"    Absolute: {imp['absolute']:.4f}")
        print(f"    Percentage: {imp['percentage']:.1f}%")
    results = {
        "num_runs": num_runs,
        "num_episodes": num_episodes,
        "with_curriculum": {"aggregated_metrics": cur_agg, "individual_metrics": cur_metrics},
        "without_curriculum": {"aggregated_metrics": no_cur_agg, "individual_metrics": no_cur_metrics},
        "improvements": improvements,
    }
    path = Path(output_dir) / "curriculum_ablation.json"
    with open(path, "w") as f:
        json.dump(results, f, indent=2)
    print(f"\nResults saved to {path}")
    print(bar)
    return results


# ------------------------------------------------------------------ the study on the policy-gradient trainer
PG_CURRICULUM_CONTRASTS = {"curriculum_effect": {"with_curriculum": 1.0, "without_curriculum": -1.0}}
# aggregate key -> (spec column, metric) of the study's group tables
_PG_AGGREGATES = {"convergence_step": ("success_rate", "x_at_convergence"),
                  "final_success_rate": ("success_rate", "final_window_mean"),
                  "best_success_rate": ("success_rate", "best"),
                  "mean_success_rate": ("success_rate", "curve_mean"),
                  "final_reward": ("mean_return", "final_window_mean"),
                  "mean_reward": ("mean_return", "curve_mean"),
                  "mean_episode_length": ("mean_length", "curve_mean")}


def pg_aggregates(result) -> Dict:
    """A ``training_study.StudyResult`` of the two arms as ``aggregate_metrics``-shaped
    dictionaries (mean and std over the runs that have the metric, None when no run does; no
    median: the device tables carry none) plus the effects paired by seed, from the validation
    slab when a validation ran, else the training slab."""
    slab = result.yardstick
    out: Dict = {}
    for arm in result.arms:
        agg = {}
        for key, (column, metric) in _PG_AGGREGATES.items():
            g = slab.group(arm, column, metric)
            agg[key] = {"mean": g["mean"], "std": g["std"]} if g["count"] > 0 else None
        agg["num_converged"] = int(slab.group(arm, "success_rate", "x_at_convergence")["count"])
        out[arm] = {"aggregated_metrics": agg}
    out["effects"] = {}
    for name in slab.contrast_names:
        out["effects"][name] = {}
        for key, (column, metric) in _PG_AGGREGATES.items():
            c = slab.contrast(name, column, metric)
            out["effects"][name][key] = ({"mean": c["mean"], "stderr": c["stderr"], "pairs": int(c["pairs"])}
                                         if c["pairs"] > 0 else None)
    return out


def run_pg_curriculum_study(iterations: int, num_runs: int = 5, *, curriculum_scheduler_config=None,
                            convergence_window: int = 10, convergence_threshold: float = 0.5, final_window: int = 10,
                            return_study: bool = False, **study_kw):
    """curriculum_ablation.py:206-357 on the policy-gradient trainer: ``num_runs`` runs (seeds 42 +
    run) with ``ablation.study_scheduler`` attached and ``num_runs`` on the fixed hard config, both
    on the dense reward, as ``training_study.run_training_study`` jobs (``study_kw`` goes there).
    Returns ``pg_aggregates``' dictionary: ``with_curriculum`` / ``without_curriculum`` and the
    paired ``effects``; with ``return_study`` also the ``StudyResult``."""
    from .ablation import pg_study_specs
    from .training_study import Arm, run_training_study
    arms = [Arm("with_curriculum", True, "dense", scheduler_config=curriculum_scheduler_config),
            Arm("without_curriculum", False, "dense")]
    specs = pg_study_specs(convergence_window, convergence_threshold, final_window)
    study_kw.setdefault("train_specs", specs)
    study_kw.setdefault("val_specs", specs)
    study_kw.setdefault("contrasts", PG_CURRICULUM_CONTRASTS)
    result = run_training_study(arms, [42 + r for r in range(int(num_runs))], iterations, **study_kw)
    out = pg_aggregates(result)
    out["num_runs"], out["iterations"] = int(num_runs), int(iterations)
    return (out, result) if return_study else out
