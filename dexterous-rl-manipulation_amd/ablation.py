"""Component-ablation drivers -- evaluation/component_ablation.py:27-408 -- on the
fused SimpleLearner rollout (``dxrl_rollout_simple``).

``train_with_config`` is the reference's sequential loop: one env instance
(sticky object), one SimpleLearner carried across ``num_episodes``
``run_episode`` calls, the learner's np.random stream seeded with ``seed``.
Every (configuration, seed) run of ``run_component_ablation`` is one device
env lane, so the whole study is one launch sequence per reward type instead
of 4 x len(seeds) Python loops.  Each lane replays the reference's streams
exactly (training.ReferenceStreams): the legacy MT19937 gauss stream of
``np.random.seed(seed)`` and the env's gymnasium PCG64 stream.  The reference
seeds that env stream from OS entropy (``env.reset()`` without a seed), so
its runs are not repeatable; ``env_seed`` pins it (None = entropy, as there).

Quirk kept: run_episode reports success = info.get("success", False) = False
(episode_utils.py:52), so the CurriculumScheduler of a curriculum run never
progresses and every success rate is 0 -- the lane keeps the scheduler's
initial configuration, exactly as the reference does.

``train_study`` / ``run_component_study`` (and ``python -m dexterous_rl_manipulation_amd.ablation``)
are the same study on ``dxrl_rollout_curriculum``: every run is a lane with a real scheduler, a
dense and a sparse ``DeviceStudy`` on two streams write one lane table, and
``dxrl_study_summarize`` reduces it to ``compute_ablation_statistics``' dictionary on the device.
There the scheduler moves whenever its rule says so (``success_rule="terminated"``, thresholds
<= 0); ``train_many`` above keeps its restriction.

``run_pg_component_study`` is the 2 x 2 on the learner this project is about: every (configuration,
seed) is one ``PGTrainer.fit`` of the MLP actor-critic (``training_study.run_training_study``), a
curriculum arm with ``study_scheduler`` attached, every run validated on the same held-out
episodes, and ``dxrl_pg_runs_summarize`` reduces the runs' device tables to the same dictionary
plus the effects paired by seed (``python -m dexterous_rl_manipulation_amd.pg_ablation``).
"""
from __future__ import annotations

import json
import os
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .envs import VecEnv
from .experiments import CurriculumConfig
from .policies import VecSimpleLearner
from .training import ReferenceStreams, SimpleLearnerRollout


@dataclass
class AblationConfig:
    """component_ablation.py:27-48."""
    use_curriculum: bool
    use_dense_reward: bool
    name: str = ""

    def __post_init__(self):
        if not self.name:
            self.name = "_".join(["curriculum" if self.use_curriculum else "no-curriculum",
                                  "dense-reward" if self.use_dense_reward else "sparse-reward"])


@dataclass
class TrainingResults:
    """component_ablation.py:51-75."""
    config: AblationConfig
    episode_rewards: List[float]
    episode_steps: List[int]
    success_rates: List[float]
    final_success_rate: float
    mean_episode_length: float
    convergence_step: Optional[int]
    total_episodes: int

    def to_dict(self) -> Dict:
        return {"config": asdict(self.config), "episode_rewards": self.episode_rewards,
                "episode_steps": self.episode_steps, "success_rates": self.success_rates,
                "final_success_rate": float(self.final_success_rate),
                "mean_episode_length": float(self.mean_episode_length),
                "convergence_step": self.convergence_step, "total_episodes": self.total_episodes}


_DIFFICULTY = {"easy": CurriculumConfig.easy, "medium": CurriculumConfig.medium, "hard": CurriculumConfig.hard}


def _lane_curriculum(cfg: AblationConfig, sched_cfg) -> CurriculumConfig:
    """component_ablation.py:97-140: a curriculum run starts (and, the scheduler never
    progressing, stays) at the scheduler's initial difficulty; otherwise the hard preset."""
    if not cfg.use_curriculum:
        return CurriculumConfig.hard()
    return _DIFFICULTY[sched_cfg.initial_difficulty if sched_cfg else "easy"]()


def _summarise(cfg: AblationConfig, rewards: np.ndarray, steps: np.ndarray, success: np.ndarray,
               num_episodes: int) -> TrainingResults:
    """component_ablation.py:168-186 (window-20 convergence, final rate over the last 20)."""
    rates = [1.0 if s else 0.0 for s in success]
    w = 20
    conv = None
    for i in range(w, len(rates)):
        if np.mean(rates[i - w:i]) >= 0.5:
            conv = i
            break
    final = np.mean(rates[-w:]) if len(rates) >= w else np.mean(rates)
    return TrainingResults(config=cfg, episode_rewards=[float(r) for r in rewards],
                           episode_steps=[int(s) for s in steps], success_rates=rates, final_success_rate=final,
                           mean_episode_length=np.mean([int(s) for s in steps]), convergence_step=conv,
                           total_episodes=num_episodes)


def _entropy_seed() -> int:
    return int(np.random.SeedSequence().entropy)


def train_many(jobs: Sequence[Tuple[AblationConfig, int]], num_episodes: int = 200, max_episode_steps: int = 200,
               learning_rate: float = 0.01, curriculum_scheduler_config=None,
               env_seeds: Optional[Sequence[Optional[int]]] = None, device=None,
               chunk_steps: int = 2048) -> Tuple[List[TrainingResults], List[int]]:
    """Every (configuration, seed) job as one env lane of fused rollouts (one env handle per
    reward type); returns the results in job order and the gauss draws each learner consumed."""
    if (curriculum_scheduler_config is not None and curriculum_scheduler_config.success_rate_threshold <= 0
            and any(c.use_curriculum for c, _ in jobs)):
        # with threshold <= 0 the reference's scheduler progresses even though training
        # episodes never report success (mean of an all-False window is 0.0 >= threshold,
        # component_ablation.py:160-170); the lanes here keep the initial difficulty
        raise ValueError("train_many assumes the ablation scheduler never progresses; "
                         "success_rate_threshold must be > 0")
    env_seeds = list(env_seeds) if env_seeds is not None else [None] * len(jobs)
    env_seeds = [_entropy_seed() if s is None else int(s) for s in env_seeds]
    results: List[Optional[TrainingResults]] = [None] * len(jobs)
    used = [0] * len(jobs)
    for dense in (True, False):
        lanes = [k for k, (c, _) in enumerate(jobs) if c.use_dense_reward == dense]
        if not lanes:
            continue
        n = len(lanes)
        env = VecEnv(n, reward_type="dense" if dense else "sparse", max_episode_steps=max_episode_steps,
                     device=device)
        idx = np.arange(n, dtype=np.int32)
        env.set_curricula([_lane_curriculum(jobs[k][0], curriculum_scheduler_config) for k in lanes], env_index=idx)
        learner = VecSimpleLearner(n, learning_rate=learning_rate, device=env.device)
        streams = ReferenceStreams(env, [env_seeds[k] for k in lanes], [jobs[k][1] for k in lanes])
        ro = SimpleLearnerRollout(env, learner, max_steps=max_episode_steps, record_cap=chunk_steps,
                                  success_rule="training", streams=streams)
        ro.start(env_index=idx)
        got: List[list] = [[] for _ in range(n)]
        remaining = np.full(n, int(num_episodes), dtype=np.int32)
        lane_used = np.zeros(n, dtype=np.int64)
        while remaining.max() > 0:
            rec = ro.run(chunk_steps, env_index=idx, episode_budget=torch.from_numpy(remaining).to(env.device))
            lane_used += ro.gauss_used.cpu().numpy()
            for j in np.lexsort((rec.end_step, rec.env_id)):  # per lane, in completion order
                got[int(rec.env_id[j])].append((rec.total_reward[j], rec.steps[j], rec.success[j]))
            counts = np.bincount(np.asarray(rec.env_id, dtype=np.int64), minlength=n)
            remaining = np.maximum(remaining - counts.astype(np.int32), 0)
        for li, k in enumerate(lanes):
            eps = got[li][:num_episodes]
            results[k] = _summarise(jobs[k][0], np.array([e[0] for e in eps], np.float64),
                                    np.array([e[1] for e in eps], np.int64), np.array([e[2] for e in eps], bool),
                                    num_episodes)
            used[k] = int(lane_used[li])
        env.close()
    return results, used


def train_with_config(config: AblationConfig, num_episodes: int = 200, max_episode_steps: int = 200,
                      seed: int = 42, learning_rate: float = 0.01, curriculum_scheduler_config=None,
                      env_seed: Optional[int] = None, device=None) -> TrainingResults:
    """component_ablation.py:78-195.  Leaves np.random where the reference leaves it:
    seeded with ``seed`` and advanced by the learner's draws."""
    (res,), (used,) = train_many([(config, seed)], num_episodes, max_episode_steps, learning_rate,
                                 curriculum_scheduler_config, [env_seed], device)
    np.random.seed(seed)
    np.random.standard_normal(used)
    return res


ABLATION_CONFIGS = [("baseline", True, True), ("no_curriculum", False, True), ("no_dense_reward", True, False),
                    ("minimal", False, False)]


def run_component_ablation(num_episodes: int = 200, max_episode_steps: int = 200, seeds: Optional[List[int]] = None,
                           learning_rate: float = 0.01, curriculum_scheduler_config=None, output_dir: str = "logs",
                           env_seeds: Optional[Dict[Tuple[str, int], int]] = None,
                           device=None) -> Dict[str, List[TrainingResults]]:
    """component_ablation.py:198-282: the four configurations x seeds as one batched run;
    results saved to <output_dir>/component_ablation_results.json."""
    seeds = [42, 123, 456] if seeds is None else list(seeds)
    configs = [AblationConfig(use_curriculum=c, use_dense_reward=d, name=nm) for nm, c, d in ABLATION_CONFIGS]
    jobs = [(c, s) for c in configs for s in seeds]
    es = [None if env_seeds is None else env_seeds.get((c.name, s)) for c, s in jobs]
    print("=" * 80)
    print("Component Ablation Study")
    print("=" * 80)
    print(f"Testing {len(configs)} configurations with {len(seeds)} seeds each")
    print(f"Episodes per run: {num_episodes}")
    print("=" * 80)
    flat, _ = train_many(jobs, num_episodes, max_episode_steps, learning_rate, curriculum_scheduler_config, es,
                         device)
    out: Dict[str, List[TrainingResults]] = {}
    for (c, _), r in zip(jobs, flat):
        out.setdefault(c.name, []).append(r)
    for c in configs:
        print(f"\nTesting: {c.name}")
        print(f"  Curriculum: {c.use_curriculum}")
        print(f"  Dense reward: {c.use_dense_reward}")
        for k, (s, r) in enumerate(zip(seeds, out[c.name])):
            print(f"  Seed {k + 1}/{len(seeds)} (seed={s})... Success rate: {r.final_success_rate:.3f}")
    os.makedirs(output_dir, exist_ok=True)
    path = Path(output_dir) / "component_ablation_results.json"
    with open(path, "w") as f:
        json.dump({k: [r.to_dict() for r in v] for k, v in out.items()}, f, indent=2)
    print(f"\nResults saved to: {path}")
    return out


def compute_ablation_statistics(all_results: Dict[str, List[TrainingResults]]) -> Dict[str, Dict]:
    """component_ablation.py:285-322."""
    stats = {}
    for name, rs in all_results.items():
        fsr = [r.final_success_rate for r in rs]
        mel = [r.mean_episode_length for r in rs]
        conv = [r.convergence_step for r in rs if r.convergence_step is not None]
        stats[name] = {
            "final_success_rate": {"mean": float(np.mean(fsr)), "std": float(np.std(fsr)),
                                   "min": float(np.min(fsr)), "max": float(np.max(fsr))},
            "mean_episode_length": {"mean": float(np.mean(mel)), "std": float(np.std(mel))},
            "convergence_step": {"mean": float(np.mean(conv)) if conv else None,
                                 "std": float(np.std(conv)) if conv else None, "num_converged": len(conv)},
        }
    return stats


# ------------------------------------------------------------------ the study on the curriculum rollout
def study_scheduler(curriculum_scheduler_config=None):
    """The scheduler of a curriculum run (component_ablation.py:101-139): the config's difficulties
    and constants, or easy -> hard with (0.3, 15, 20, 5)."""
    from .experiments import CurriculumScheduler
    c = curriculum_scheduler_config
    if c is None:
        return CurriculumScheduler(initial_config=CurriculumConfig.easy(), target_config=CurriculumConfig.hard(),
                                   success_rate_threshold=0.3, window_size=15, min_episodes_before_progression=20,
                                   progression_steps=5)
    return CurriculumScheduler(initial_config=_DIFFICULTY[c.initial_difficulty](),
                               target_config=_DIFFICULTY[c.target_difficulty](),
                               success_rate_threshold=c.success_rate_threshold, window_size=c.window_size,
                               min_episodes_before_progression=c.min_episodes_before_progression,
                               progression_steps=c.progression_steps)


def train_study(jobs: Sequence[Tuple[AblationConfig, int]], num_episodes: int = 200, max_episode_steps: int = 200,
                learning_rate: float = 0.01, curriculum_scheduler_config=None, success_rule: str = "training",
                device_streams: bool = False, env_seeds: Optional[Sequence[Optional[int]]] = None, device=None,
                stream_seed: int = 0):
    """Every (configuration, seed) job as one lane of ``dxrl_rollout_curriculum``: a ``DeviceStudy``
    per reward type (dense first), each one launch on a stream of its own, the curriculum lanes with
    a real scheduler (so it moves when its rule says so: thresholds <= 0 and
    ``success_rule="terminated"`` work).  Nothing is copied to the host.  Returns ``(studies,
    lane_of_job)``: ``lane_of_job[k]`` is job k's row in the lane table ``summarize_runs(studies,
    ...)`` writes.  The caller closes the studies."""
    from . import curriculum_ablation as CA
    from . import _native as N
    dev = N.require_gpu(device)
    sched, hard = study_scheduler(curriculum_scheduler_config), CurriculumConfig.hard()
    es = list(env_seeds) if env_seeds is not None else [None] * len(jobs)
    studies, lane_of_job, base = [], [0] * len(jobs), 0
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(dev))
    try:
        for dense in (True, False):
            lanes = [k for k, (c, _) in enumerate(jobs) if c.use_dense_reward == dense]
            if not lanes:
                continue
            side = torch.cuda.Stream(dev)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                st = CA.launch_runs([(sched if jobs[k][0].use_curriculum else hard, jobs[k][1]) for k in lanes],
                                    num_episodes, max_episode_steps, learning_rate, success_rule,
                                    [es[k] for k in lanes], dev, "dense" if dense else "sparse", device_streams,
                                    stream_seed)
                st.launched = torch.cuda.Event()
                st.launched.record(side)
            studies.append(st)
            for j, k in enumerate(lanes):
                lane_of_job[k] = base + j
            base += len(lanes)
    except Exception:
        for st in studies:
            st.close()
        raise
    return studies, lane_of_job


def run_component_study(num_episodes: int = 200, max_episode_steps: int = 200, seeds: Optional[List[int]] = None,
                        learning_rate: float = 0.01, curriculum_scheduler_config=None,
                        success_rule: str = "training", device_streams: bool = False,
                        env_seeds: Optional[Dict[Tuple[str, int], int]] = None, device_summary: bool = True,
                        return_runs: bool = False, output_dir: Optional[str] = None, device=None):
    """component_ablation.py:198-322 on ``train_study``: the four configurations x seeds as lanes
    of two launches writing one lane table, reduced by ``dxrl_study_summarize`` to
    ``compute_ablation_statistics``' dictionary (from ``group_stats``), which feeds
    ``print_ablation_report``.  ``device_summary=False`` copies the episode records and summarises
    on the host instead (same dictionary).  ``return_runs=True`` also returns ``{name:
    [TrainingResults per seed]}`` (this copies the records); ``output_dir`` writes the reference's
    component_ablation_results.json, which needs the runs."""
    from . import curriculum_ablation as CA
    seeds = [42, 123, 456] if seeds is None else list(seeds)
    configs = [AblationConfig(use_curriculum=c, use_dense_reward=d, name=nm) for nm, c, d in ABLATION_CONFIGS]
    jobs = [(c, s) for c in configs for s in seeds]
    es = [None if env_seeds is None else env_seeds.get((c.name, s)) for c, s in jobs]
    want_runs = return_runs or output_dir is not None or not device_summary
    studies, lane = train_study(jobs, num_episodes, max_episode_steps, learning_rate, curriculum_scheduler_config,
                                success_rule, device_streams, es, device)
    try:
        stats = None
        if device_summary:
            groups = {c.name: [lane[k] for k, (cj, _) in enumerate(jobs) if cj is c] for c in configs}
            stats = CA.summarize_runs(studies, groups)["statistics"]
        out: Dict[str, List[TrainingResults]] = {}
        if want_runs:
            CA.BYTES_COPIED["records"] = 0
            for st in studies:
                done = getattr(st, "launched", None)
                if done is not None:
                    torch.cuda.current_stream(st.device).wait_event(done)
                st.check_status()
            recs = [r for st in studies for r in st.records()]
            for k, (c, _) in enumerate(jobs):
                r = recs[lane[k]]
                out.setdefault(c.name, []).append(_summarise(c, r["reward"], r["steps"], r["success"], num_episodes))
        if stats is None:
            stats = compute_ablation_statistics(out)
    finally:
        for st in studies:
            st.close()
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        path = Path(output_dir) / "component_ablation_results.json"
        with open(path, "w") as f:
            json.dump({k: [r.to_dict() for r in v] for k, v in out.items()}, f, indent=2)
        print(f"\nResults saved to: {path}")
    return (stats, out) if return_runs else stats


# ------------------------------------------------------------------ the study on the policy-gradient trainer
# the 2 x 2 as contrasts over the four arms (weights per arm; runs paired by seed): both main
# effects, the interaction, and every arm against the baseline
PG_COMPONENT_CONTRASTS = {
    "curriculum_effect": {"baseline": 0.5, "no_dense_reward": 0.5, "no_curriculum": -0.5, "minimal": -0.5},
    "dense_reward_effect": {"baseline": 0.5, "no_curriculum": 0.5, "no_dense_reward": -0.5, "minimal": -0.5},
    "interaction": {"baseline": 1.0, "no_curriculum": -1.0, "no_dense_reward": -1.0, "minimal": 1.0},
    "no_curriculum_vs_baseline": {"no_curriculum": 1.0, "baseline": -1.0},
    "no_dense_reward_vs_baseline": {"no_dense_reward": 1.0, "baseline": -1.0},
    "minimal_vs_baseline": {"minimal": 1.0, "baseline": -1.0},
}


def pg_component_arms(curriculum_scheduler_config=None):
    """The four ``ABLATION_CONFIGS`` as arms of a ``training_study``: a curriculum arm trains under
    ``study_scheduler(curriculum_scheduler_config)``, the others on the hard preset."""
    from .training_study import Arm
    return [Arm(nm, c, "dense" if d else "sparse", scheduler_config=curriculum_scheduler_config)
            for nm, c, d in ABLATION_CONFIGS]


def pg_study_specs(window: int = 10, threshold: float = 0.5, final_window: int = 10):
    """The specs both slabs of a PG ablation are reduced with: the success rate (its final window
    and its convergence, reported in env steps), the mean episode length and the mean return."""
    from .training_study import Spec
    return tuple(Spec(c, "env_steps", int(window), float(threshold), int(final_window))
                 for c in ("success_rate", "mean_length", "mean_return"))


def _none_if_nan(x: float):
    return None if np.isnan(x) else float(x)


def pg_statistics(result, effects: bool = True) -> Dict[str, Dict]:
    """``compute_ablation_statistics``' dictionary from a ``StudyResult``'s group tables -- the
    validation slab's when a validation ran, else the training slab's: ``final_success_rate`` is
    the final-window mean of ``success_rate``, ``mean_episode_length`` the curve mean of
    ``mean_length``, ``convergence_step`` the env steps at the convergence of ``success_rate`` over
    the runs that converged.  With ``effects``, an ``"effects"`` entry holds, per contrast, the
    mean, standard error and pair count of the paired final success rate."""
    slab = result.yardstick
    stats: Dict[str, Dict] = {}
    for arm in result.arms:
        fsr = slab.group(arm, "success_rate", "final_window_mean")
        mel = slab.group(arm, "mean_length", "curve_mean")
        conv = slab.group(arm, "success_rate", "x_at_convergence")
        stats[arm] = {
            "final_success_rate": {k: fsr[k] for k in ("mean", "std", "min", "max")},
            "mean_episode_length": {k: mel[k] for k in ("mean", "std")},
            "convergence_step": {"mean": _none_if_nan(conv["mean"]), "std": _none_if_nan(conv["std"]),
                                 "num_converged": int(conv["count"])},
        }
    if effects:
        stats["effects"] = {}
        for name in slab.contrast_names:
            c = slab.contrast(name, "success_rate", "final_window_mean")
            stats["effects"][name] = {"mean": c["mean"], "stderr": c["stderr"], "pairs": int(c["pairs"])}
    return stats


def run_pg_component_study(iterations: int, seeds: Sequence[int] = (42, 123, 456), *, curriculum_scheduler_config=None,
                           convergence_window: int = 10, convergence_threshold: float = 0.5, final_window: int = 10,
                           return_study: bool = False, **study_kw):
    """component_ablation.py:198-322 on the policy-gradient trainer: the four configurations x
    seeds as ``training_study.run_training_study`` jobs (``study_kw`` goes there: num_envs,
    horizon, max_steps, heldout_set, validate_every, val_episodes, device_summary, ...), reduced by
    ``dxrl_pg_runs_summarize`` to ``compute_ablation_statistics``' dictionary plus ``"effects"``
    (``pg_statistics``), which feeds ``print_ablation_report``.  ``return_study=True`` also returns
    the ``StudyResult``."""
    from .training_study import run_training_study
    specs = pg_study_specs(convergence_window, convergence_threshold, final_window)
    study_kw.setdefault("train_specs", specs)
    study_kw.setdefault("val_specs", specs)
    study_kw.setdefault("contrasts", PG_COMPONENT_CONTRASTS)
    result = run_training_study(pg_component_arms(curriculum_scheduler_config), list(seeds), iterations, **study_kw)
    stats = pg_statistics(result)
    return (stats, result) if return_study else stats


def main(argv: Optional[Sequence[str]] = None):
    """evaluation/run_component_ablation.py:24-102 on ``run_component_study`` (plots are not part of
    this build: the reference's warning line is printed in their place)."""
    import argparse
    from .experiments import load_config, load_named_config
    parser = argparse.ArgumentParser(description="Run component ablation study")
    parser.add_argument("--config", type=str, default=None,
                        help="Path to experiment configuration JSON file (default: use default config)")
    parser.add_argument("--config-name", type=str, default=None,
                        help="Name of predefined configuration (e.g., 'default', 'quick_test')")
    parser.add_argument("--success-rule", choices=("training", "terminated"), default="training",
                        help="training: success as run_episode reports it (always False); terminated: the episode "
                             "terminated")
    parser.add_argument("--device-streams", action="store_true",
                        help="per-run Philox streams on the device instead of the reference's host streams")
    args = parser.parse_args(argv)
    if args.config_name:
        exp_config = load_named_config(args.config_name)
    elif args.config:
        exp_config = load_config(args.config)
    else:
        exp_config = load_config()
    ab = exp_config.component_ablation
    bar = "=" * 80
    print(bar)
    print("Component Ablation Study")
    print(bar)
    print(f"Experiment: {exp_config.experiment_name}")
    if exp_config.description:
        print(f"Description: {exp_config.description}")
    print("\nThis study tests all combinations of:")
    print("  - Curriculum learning (on/off)")
    print("  - Dense reward shaping (on/off)")
    print("\nConfigurations tested:")
    print("  1. Baseline: Curriculum + Dense Reward")
    print("  2. No Curriculum: Fixed difficulty + Dense Reward")
    print("  3. No Dense Reward: Curriculum + Sparse Reward")
    print("  4. Minimal: Fixed difficulty + Sparse Reward")
    print(bar)
    print("\nConfiguration:")
    print(f"  Episodes per run: {ab.num_episodes}")
    print(f"  Max episode steps: {ab.max_episode_steps}")
    print(f"  Seeds: {ab.seeds}")
    print(f"  Learning rate: {ab.learning_rate}")
    print(bar)
    stats, all_results = run_component_study(
        num_episodes=ab.num_episodes, max_episode_steps=ab.max_episode_steps, seeds=ab.seeds,
        learning_rate=ab.learning_rate, curriculum_scheduler_config=ab.curriculum_scheduler,
        success_rule=args.success_rule, device_streams=args.device_streams, return_runs=True,
        output_dir=exp_config.output_dir)
    print_ablation_report(all_results, stats)
    print("\nGenerating visualizations...")
    print("Warning: Could not generate plots: plotting is not part of this build")
    print("\n" + bar)
    print("Component Ablation Study Complete")
    print(bar)
    print(f"\nResults saved to: {Path(exp_config.output_dir) / 'component_ablation_results.json'}")
    print(bar)
    return stats


def print_ablation_report(all_results: Dict[str, List[TrainingResults]], stats: Dict[str, Dict]):
    """component_ablation.py:325-408 (same text)."""
    bar, rule = "=" * 80, "-" * 80
    base_name = "baseline" if "baseline" in stats else list(stats)[0]
    base = stats[base_name]["final_success_rate"]["mean"]
    lines = ["\n" + bar, "Component Ablation Report", bar, "\nBaseline (Curriculum + Dense Reward):",
             f"  Final Success Rate: {base:.3f} +/- {stats[base_name]['final_success_rate']['std']:.3f}",
             "\n" + rule, "Component Contributions:", rule]
    for name, st in stats.items():
        if name == base_name or name == "effects":  # "effects": pg_statistics' contrasts, not a configuration
            continue
        m, sd = st["final_success_rate"]["mean"], st["final_success_rate"]["std"]
        diff = m - base
        pct = (diff / base * 100) if base > 0 else 0
        lines += [f"\n{name.replace('_', ' ').title()}:", f"  Final Success Rate: {m:.3f} +/- {sd:.3f}",
                  f"  Difference from baseline: {diff:+.3f} ({pct:+.1f}%)"]
        c = st["convergence_step"]
        lines.append(f"  Convergence step: {c['mean']:.0f} +/- {c['std']:.0f}" if c["mean"] is not None
                     else "  Convergence: Not reached")
    lines += ["\n" + rule, "Key Insights:", rule]
    insights = [("no_curriculum", "Curriculum Learning Impact", "Without curriculum", "With curriculum", "Improvement"),
                ("no_dense_reward", "Dense Reward Impact", "Without dense reward", "With dense reward", "Improvement"),
                ("minimal", "Combined Impact", "Minimal (no curriculum, sparse reward)",
                 "Full system (curriculum + dense reward)", "Total improvement")]
    for k, (name, title, without, with_, label) in enumerate(insights, 1):
        if name not in stats:
            continue
        other = stats[name]["final_success_rate"]["mean"]
        d = base - other
        pct = (d / base * 100) if base > 0 else 0
        lines += [f"\n{k}. {title}:", f"   {without}: {other:.3f}", f"   {with_}: {base:.3f}",
                  f"   {label}: {d:+.3f} ({pct:+.1f}%)"]
    lines.append("\n" + bar)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
