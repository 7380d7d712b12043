"""Seed-variance analysis -- evaluation/seed_variance.py:18-196,288-446 and
evaluation/run_seed_variance.py, on the device evaluator.

Same names, signatures, result dictionaries, report text and files
(``seed_variance_analysis.json``, ``seed_variance.png``) as the reference.  Two
execution forms:

* exact order (default) -- the reference's loop, one
  ``Evaluator.evaluate_heldout_set(seed=s)`` per seed.  The policy's global
  random stream runs on from seed to seed (the evaluator commits what each run
  consumed), so the results equal the reference's bit for bit
  (tests/golden/seed_variance_golden.json).
* ``parallel=True`` -- the whole study is ONE episode launch, one lane per
  (seed, object, episode) with reset seed ``seed + k`` as ``heldout_program``
  lays it out, and ONE ``dxrl_eval_summarize`` launch with the groups
  (seed, object), seed and overall; only the group tables cross to the host.
  ``policy_seeds`` (one per lane) replays per-episode policy streams and the
  host reset draws of those seeds; without it the lanes run device Philox
  streams keyed by (``device_seed``, lane), where a seed's episodes differ from
  another's by their lanes, not by the seed's value.  ``results_by_seed[s]``
  has the shape of ``evaluate_heldout_set(device_summary=True)``.

Reference quirk, kept: ``compute_variance_statistics`` reads
``overall_success_rate`` and ``mean_reward`` from ``results["metrics"]``, which
has neither key, so both statistics are all zeros (seed_variance.py:127,138).
``extended=True`` adds a separate ``variance_stats_extended`` computed from
``overall_stats``; the reference's keys stay as they are.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np

from .experiments import ExperimentConfig, SeedVarianceConfig

# metric key -> where the reference looks it up (always results["metrics"], see the quirk above)
_METRIC_KEYS = ("grasp_success_rate", "mean_episode_length", "overall_success_rate", "mean_reward")
_BAR = "=" * 60


def _spread(values: List) -> Dict:
    """mean / std / min / max / coefficient of variation of one metric's per-seed values."""
    mean, std = np.mean(values), np.std(values)
    return {"mean": float(mean), "std": float(std), "min": float(np.min(values)), "max": float(np.max(values)),
            "cv": float(std / mean) if mean > 0 else 0.0, "values": values}


class SeedVarianceAnalyzer:
    """seed_variance.py:18-196."""

    def __init__(self, policy, heldout_set, reward_type: str = "dense", max_episode_steps: int = 200, device=None):
        self.policy = policy
        self.heldout_set = heldout_set
        self.reward_type = reward_type
        self.max_episode_steps = max_episode_steps
        self.device = device
        self.last_summary = None  # parallel form: the study's EvalSummary (last group = all episodes)

    def _evaluator(self):
        from .evaluator import Evaluator
        return Evaluator(policy=self.policy, heldout_set=self.heldout_set, reward_type=self.reward_type,
                         max_episode_steps=self.max_episode_steps, device=self.device)

    def evaluate_multiple_seeds(self, seeds: List[int], num_episodes_per_object: int = 5, parallel: bool = False,
                                policy_seeds: Optional[Sequence[int]] = None, device_seed: int = 0,
                                timing: Optional[Dict] = None) -> Dict:
        """seed_variance.py:44-78; ``parallel=True`` runs the study as one launch (module docstring)."""
        if parallel:
            return self._one_launch(list(seeds), int(num_episodes_per_object), policy_seeds, device_seed, timing)
        results_by_seed = {}
        for seed in seeds:
            print(f"  Evaluating with seed {seed}...")
            results_by_seed[seed] = self._evaluator().evaluate_heldout_set(
                num_episodes_per_object=num_episodes_per_object, seed=seed)
        return results_by_seed

    def _one_launch(self, seeds, K, policy_seeds, device_seed, timing) -> Dict:
        from . import _native as N
        from .evaluator import _seeded_tapes, compiled_program
        ev = self._evaluator()
        n_obj = len(self.heldout_set.heldout_objects)
        if n_obj > N.MAX_CURRICULA:
            raise ValueError(f"a one-launch study holds every held-out object as a curriculum row of one launch: "
                             f"{n_obj} objects exceed DXRL_MAX_CURRICULA = {N.MAX_CURRICULA}; use parallel=False")
        prog = compiled_program(self.policy)
        if prog is None:
            raise ValueError("parallel=True needs a policy the episode kernel compiles")
        ev.freeze_policy()
        program = None
        for seed in seeds:
            print(f"  Evaluating with seed {seed}...")
            p = ev.heldout_program(K, seed, parallel=True)
            if program is None:
                program = p
            else:
                program.lanes += p.lanes
        per_seed = n_obj * K
        S = len(seeds)
        groups = [np.arange(si * per_seed + o * K, si * per_seed + (o + 1) * K) for si in range(S)
                  for o in range(n_obj)]
        groups += [np.arange(si * per_seed, (si + 1) * per_seed) for si in range(S)]
        groups.append(np.arange(S * per_seed))
        if policy_seeds is not None:
            summ = program.run(prog, policy_tapes=_seeded_tapes(prog, program, policy_seeds), groups=groups,
                               timing=timing)
        else:
            summ = program.run(prog, host_resets=False, host_noise=False, device_seed=device_seed, groups=groups,
                               timing=timing)
        self.last_summary = summ
        out = {}
        for si, seed in enumerate(seeds):
            res = ev.summary_results(summ, K, object_groups=range(si * n_obj, (si + 1) * n_obj),
                                     overall_group=S * n_obj + si)
            del res["summary"]  # one table for the whole study: self.last_summary
            out[seed] = res
        return out

    def compute_variance_statistics(self, results_by_seed: Dict, extended: bool = False) -> Dict:
        """seed_variance.py:80-153."""
        seeds = list(results_by_seed.keys())
        per_seed = [r.get("metrics", {}) for r in results_by_seed.values()]
        stats = {key: _spread([m.get(key, 0.0) for m in per_seed]) for key in _METRIC_KEYS}
        out = {"seeds": seeds, "num_seeds": len(seeds), "variance_stats": stats,
               "individual_results": results_by_seed}
        if extended:
            overall = [r.get("overall_stats", {}) for r in results_by_seed.values()]
            out["variance_stats_extended"] = {key: _spread([o.get(key, 0.0) for o in overall])
                                              for key in ("overall_success_rate", "mean_reward")}
        return out

    def validate_variance(self, variance_stats: Dict, max_cv_threshold: float = 0.2) -> Dict[str, Dict]:
        """seed_variance.py:155-196."""
        out = {}
        for name, st in variance_stats.items():
            cv, std, mean = st.get("cv", 0.0), st.get("std", 0.0), st.get("mean", 0.0)
            rel = (std / abs(mean)) if mean != 0 else 0.0
            cv_ok, rel_ok = cv <= max_cv_threshold, rel <= max_cv_threshold
            out[name] = {"is_controlled": cv_ok and rel_ok, "cv": cv, "cv_threshold": max_cv_threshold,
                         "cv_ok": cv_ok, "relative_std": rel, "relative_std_ok": rel_ok}
        return out


def plot_seed_variance(variance_analysis: Dict, output_path: str = "logs/seed_variance.png") -> None:
    """seed_variance.py:199-285: per-seed success rate and episode length with their mean and
    +-1 std band, a box plot of three metrics, and the coefficient of variation of each."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    stats, seeds = variance_analysis["variance_stats"], variance_analysis["seeds"]
    fig, axes = plt.subplots(2, 2, figsize=(14, 10))
    panels = [(axes[0, 0], "grasp_success_rate", "o-", None, "Success Rate", "Grasp Success Rate",
               "Success Rate Variance Across Seeds", ".3f"),
              (axes[0, 1], "mean_episode_length", "s-", "orange", "Mean Episode Length",
               "Mean Episode Length (steps)", "Episode Length Variance Across Seeds", ".1f")]
    for ax, key, marker, color, label, ylabel, title, fmt in panels:
        st = stats[key]
        ax.plot(seeds, st["values"], marker, linewidth=2, markersize=8, label=label,
                **({"color": color} if color else {}))
        ax.axhline(st["mean"], color="r", linestyle="--", alpha=0.7, label=f"Mean: {st['mean']:{fmt}}")
        ax.fill_between(seeds, st["mean"] - st["std"], st["mean"] + st["std"], alpha=0.2, color="red",
                        label=f"±1 std: {st['std']:{fmt}}")
        ax.set_xlabel("Seed")
        ax.set_ylabel(ylabel)
        ax.set_title(title)
        ax.legend()
        ax.grid(True, alpha=0.3)
    axes[0, 0].set_ylim([0, 1.1])

    ax = axes[1, 0]
    boxed = ["grasp_success_rate", "mean_episode_length", "overall_success_rate"]
    bp = ax.boxplot([stats[m]["values"] for m in boxed], patch_artist=True)
    ax.set_xticklabels(["Success Rate", "Episode Length", "Overall Success"])
    for box, color in zip(bp["boxes"], ("lightblue", "lightcoral", "lightgreen")):
        box.set_facecolor(color)
    ax.set_ylabel("Value")
    ax.set_title("Metric Distribution Across Seeds")
    ax.tick_params(axis="x", rotation=45)
    ax.grid(True, alpha=0.3, axis="y")

    ax = axes[1, 1]
    names = list(stats.keys())
    cvs = [stats[m]["cv"] for m in names]
    bars = ax.bar(names, cvs, color=["green" if c <= 0.2 else "orange" if c <= 0.5 else "red" for c in cvs],
                  alpha=0.7)
    ax.axhline(0.2, color="r", linestyle="--", label="Threshold (0.2)", alpha=0.7)
    ax.set_xlabel("Metric")
    ax.set_ylabel("Coefficient of Variation")
    ax.set_title("Variance Stability (CV)")
    ax.tick_params(axis="x", rotation=45)
    ax.legend()
    ax.grid(True, alpha=0.3, axis="y")
    for bar, cv in zip(bars, cvs):
        ax.text(bar.get_x() + bar.get_width() / 2.0, bar.get_height(), f"{cv:.3f}", ha="center", va="bottom")

    fig.tight_layout()
    fig.savefig(output_path, dpi=150)
    plt.close(fig)
    print(f"Seed variance plot saved to {output_path}")


def print_variance_report(variance_analysis: Dict, validation: Dict):
    """seed_variance.py:288-332, line for line."""
    seeds, stats = variance_analysis["seeds"], variance_analysis["variance_stats"]
    lines = ["\n" + _BAR, "Seed Variance Analysis Report", _BAR, f"\nSeeds tested: {seeds}",
             f"Number of seeds: {len(seeds)}", "\nVariance Statistics:"]
    for name, st in stats.items():
        lines += [f"\n  {name}:", f"    Mean: {st['mean']:.4f}", f"    Std:  {st['std']:.4f}",
                  f"    Min:  {st['min']:.4f}", f"    Max:  {st['max']:.4f}",
                  f"    CV:   {st['cv']:.4f} (Coefficient of Variation)"]
        if name in validation:
            v = validation[name]
            lines.append(f"    Status: {'[PASS]' if v['is_controlled'] else '[FAIL]'} "
                         f"(CV threshold: {v['cv_threshold']})")
    lines.append("\nValidation Summary:")
    for name, v in validation.items():
        lines.append(f"  {name}: {'CONTROLLED' if v['is_controlled'] else 'HIGH VARIANCE'} (CV: {v['cv']:.4f})")
    if all(v["is_controlled"] for v in validation.values()):
        lines.append("\n[PASS] All metrics show controlled variance across seeds")
    else:
        lines.append("\n[WARNING] Some metrics show high variance across seeds")
    lines.append(_BAR)
    print("\n".join(lines))


def _jsonable(x):
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, (np.bool_, bool)):
        return bool(x)
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    if isinstance(x, np.ndarray):
        return x.tolist()
    return x


def analyze_seed_variance(policy, heldout_set, seeds: List[int], num_episodes_per_object: int = 5,
                          reward_type: str = "dense", max_episode_steps: int = 200, output_dir: str = "logs",
                          max_cv_threshold: float = 0.2, parallel: bool = False,
                          policy_seeds: Optional[Sequence[int]] = None, device_seed: int = 0,
                          extended: bool = False, device=None) -> Dict:
    """seed_variance.py:335-446: evaluate every seed, compute and validate the spread, print the
    report, write ``seed_variance.png`` and ``seed_variance_analysis.json`` under ``output_dir``."""
    print(_BAR)
    print("Seed Variance Analysis")
    print(_BAR)
    if len(seeds) < 3:
        raise ValueError("At least 3 seeds required for variance analysis")
    print(f"\nEvaluating with {len(seeds)} seeds: {seeds}")
    analyzer = SeedVarianceAnalyzer(policy=policy, heldout_set=heldout_set, reward_type=reward_type,
                                    max_episode_steps=max_episode_steps, device=device)
    print("\n1. Running evaluations with multiple seeds...")
    extra: Dict[str, Any] = dict(parallel=True, policy_seeds=policy_seeds, device_seed=device_seed) if parallel else {}
    results_by_seed = analyzer.evaluate_multiple_seeds(seeds=seeds, num_episodes_per_object=num_episodes_per_object,
                                                       **extra)
    print("\n2. Computing variance statistics...")
    analysis = analyzer.compute_variance_statistics(results_by_seed, **({"extended": True} if extended else {}))
    print("\n3. Validating variance...")
    validation = analyzer.validate_variance(analysis["variance_stats"], max_cv_threshold=max_cv_threshold)
    print_variance_report(analysis, validation)
    print("\n4. Generating visualizations...")
    os.makedirs(output_dir, exist_ok=True)
    plot_seed_variance(analysis, os.path.join(output_dir, "seed_variance.png"))
    print("\n5. Saving results...")
    results_path = os.path.join(output_dir, "seed_variance_analysis.json")
    with open(results_path, "w") as f:
        json.dump({"variance_analysis": _jsonable(analysis), "validation": _jsonable(validation)}, f, indent=2)
    print(f"   Results saved to {results_path}")
    print("\n" + _BAR)
    print("Seed Variance Analysis Complete")
    print(_BAR)
    return {"variance_analysis": analysis, "validation": validation}


def run_seed_variance(config: Union[SeedVarianceConfig, ExperimentConfig], policy, heldout_set,
                      output_dir: str = "logs", parallel: bool = False, **kwargs) -> Dict:
    """``analyze_seed_variance`` with the fields of a ``SeedVarianceConfig`` (or of the
    ``seed_variance`` section of an ``ExperimentConfig``)."""
    c = config.seed_variance if isinstance(config, ExperimentConfig) else config
    return analyze_seed_variance(policy, heldout_set, seeds=list(c.seeds),
                                 num_episodes_per_object=c.num_episodes_per_object, reward_type=c.reward_type,
                                 max_episode_steps=c.max_episode_steps, output_dir=output_dir,
                                 max_cv_threshold=c.max_cv_threshold, parallel=parallel, **kwargs)


def main():
    """evaluation/run_seed_variance.py: RandomPolicy on 10 held-out objects of the medium
    curriculum, the reference's seven seeds, 5 episodes per object."""
    from . import envs, evaluation, policies
    from .experiments import CurriculumConfig
    print(_BAR)
    print("Seed Variance Analysis Example")
    print(_BAR)
    print("\n1. Setting up evaluation...")
    train_config = CurriculumConfig.medium()
    heldout_set = evaluation.HeldOutObjectSet(train_config, num_heldout_objects=10, seed=42)
    env = envs.DexterousManipulationEnv(curriculum_config=train_config)
    policy = policies.RandomPolicy(env.action_space, seed=42)
    env.close()
    seeds = [42, 123, 456, 789, 1000, 2024, 3000]
    print(f"\n2. Testing with {len(seeds)} seeds: {seeds}")
    print("\n3. Running seed variance analysis...")
    res = analyze_seed_variance(policy=policy, heldout_set=heldout_set, seeds=seeds, num_episodes_per_object=5,
                                reward_type="dense", max_episode_steps=200, output_dir="logs", max_cv_threshold=0.2)
    stats, validation = res["variance_analysis"]["variance_stats"], res["validation"]
    print("\n" + _BAR)
    print("Analysis Summary")
    print(_BAR)
    print(f"\nSeeds tested: {len(res['variance_analysis']['seeds'])}")
    for key, label, fmt in (("grasp_success_rate", "Grasp Success Rate", ".3f"),
                            ("mean_episode_length", "Mean Episode Length", ".1f")):
        st = stats[key]
        print(f"\n  {label}:\n    Mean: {st['mean']:{fmt}}\n    Std:  {st['std']:{fmt}}\n    CV:   {st['cv']:.4f}")
    controlled = sum(1 for v in validation.values() if v["is_controlled"])
    print(f"\nVariance Validation:\n  {controlled}/{len(validation)} metrics show controlled variance")
    print(_BAR)


__all__ = ["SeedVarianceAnalyzer", "plot_seed_variance", "print_variance_report", "analyze_seed_variance",
           "run_seed_variance"]

if __name__ == "__main__":
    main()
