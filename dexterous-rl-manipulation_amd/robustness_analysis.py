"""Robustness analysis: evaluation/robustness_analysis.py, and the same study on the device.

* ``analyze_robustness_results`` / ``print_robustness_report`` / ``plot_robustness_results``
  -- robustness_analysis.py:12-201 on the result of any ``RobustnessTester.run_robustness_sweep``
  (host or device summarised): the reference's signatures, dictionary keys in its order, printed
  text and four-panel figure.
* ``run_robustness_study`` -- the sweep and its analysis as one episode launch without a
  contact history plus one ``dxrl_robustness_summarize`` (csrc/dxrl_robustness_summary.hip):
  one group per noise level in ``RobustnessTester.sweep_levels`` order, every level compared
  with group 0, and the degradation columns formed on the device with the reference's f64
  operations.  Only the group tables (128 + 32 bytes per level) cross to the host: the
  analysis reads no reward moments, and the per-lane draw counts cross only in exact order,
  where the host policy stream is advanced by them.  Tie rows
  of the variance rule stay as the exact integer comparison decides them (not unstable): there
  is no history row np.var could be asked about; ``summary.tie_rows`` lists them.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np

_FAMILIES = ("observation_noise", "dynamics_noise", "combined_noise")


def _pyplot():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def _degradation_row(baseline_success: float, metrics: Dict) -> Dict:
    rate = metrics["grasp_success_rate"]
    degradation = baseline_success - rate
    pct = (degradation / baseline_success * 100) if baseline_success > 0 else 0.0
    return {"success_rate": rate, "degradation": degradation, "degradation_percentage": pct,
            "mean_episode_length": metrics["mean_episode_length"]}


def analyze_robustness_results(results: Dict) -> Dict:
    """robustness_analysis.py:12-77: every level's success rate against the baseline's."""
    base = results["baseline"]["metrics"]
    rate = base["grasp_success_rate"]
    analysis: Dict[str, Any] = {"baseline": {"success_rate": rate,
                                             "mean_episode_length": base["mean_episode_length"]}}
    for fam in _FAMILIES:
        analysis[f"{fam}_degradation"] = {k: _degradation_row(rate, r["metrics"]) for k, r in results[fam].items()}
    return analysis


def plot_robustness_results(results: Dict, analysis: Dict, output_path: str = "logs/robustness_analysis.png"):
    """robustness_analysis.py:80-168: success rate against observation and dynamics noise, both
    degradation curves, and the combined-noise heat map when the sweep has combined levels."""
    plt = _pyplot()
    fig, axes = plt.subplots(2, 2, figsize=(14, 10))
    baseline = analysis["baseline"]["success_rate"]
    curves = {}
    panels = (("observation_noise", axes[0, 0], "o-", None, "Observation"),
              ("dynamics_noise", axes[0, 1], "s-", "orange", "Dynamics"))
    for fam, ax, marker, color, word in panels:
        table = analysis[f"{fam}_degradation"]
        levels = sorted(table.keys())
        curves[fam] = (levels, [table[k]["degradation_percentage"] for k in levels])
        kw = {"color": color} if color else {}
        ax.plot(levels, [table[k]["success_rate"] for k in levels], marker, label="Success Rate", linewidth=2, **kw)
        ax.axhline(baseline, color="r", linestyle="--", label="Baseline", alpha=0.7)
        ax.set_xlabel(f"{word} Noise Std")
        ax.set_ylabel("Success Rate")
        ax.set_title(f"Robustness to {word} Noise")
        ax.legend()
        ax.grid(True, alpha=0.3)
        ax.set_ylim([0, 1.1])
    ax = axes[1, 0]
    ax.plot(*curves["observation_noise"], "o-", label="Observation Noise", linewidth=2)
    ax.plot(*curves["dynamics_noise"], "s-", label="Dynamics Noise", linewidth=2, color="orange")
    ax.set_xlabel("Noise Std")
    ax.set_ylabel("Performance Degradation (%)")
    ax.set_title("Performance Degradation vs Noise Level")
    ax.legend()
    ax.grid(True, alpha=0.3)
    ax = axes[1, 1]
    combined = analysis["combined_noise_degradation"]
    if combined:
        cells = {(float(k.split("_")[1]), float(k.split("_")[3])): v["degradation_percentage"]
                 for k, v in combined.items()}
        obs = sorted({o for o, _ in cells})
        dyn = sorted({d for _, d in cells})
        grid = np.zeros((len(dyn), len(obs)))
        for (o, d), v in cells.items():
            grid[dyn.index(d), obs.index(o)] = v
        im = ax.imshow(grid, aspect="auto", cmap="Reds", origin="lower")
        ax.set_xticks(range(len(obs)))
        ax.set_xticklabels([f"{x:.2f}" for x in obs])
        ax.set_yticks(range(len(dyn)))
        ax.set_yticklabels([f"{x:.2f}" for x in dyn])
        ax.set_xlabel("Observation Noise Std")
        ax.set_ylabel("Dynamics Noise Std")
        ax.set_title("Combined Noise Degradation (%)")
        plt.colorbar(im, ax=ax)
    else:
        ax.text(0.5, 0.5, "No combined noise data", ha="center", va="center", transform=ax.transAxes)
        ax.set_title("Combined Noise (Not Available)")
    plt.tight_layout()
    plt.savefig(output_path, dpi=150)
    plt.close(fig)
    print(f"Robustness analysis plot saved to {output_path}")


def print_robustness_report(analysis: Dict):
    """robustness_analysis.py:171-201."""
    rule = "=" * 60
    print("\n" + rule)
    print("Robustness Analysis Report")
    print(rule)
    base = analysis["baseline"]
    print("\nBaseline Performance (No Noise):")
    print(f"  Success rate: {base['success_rate']:.1%}")
    print(f"  Mean episode length: {base['mean_episode_length']:.1f} steps")
    for title, fam in (("Observation", "observation_noise"), ("Dynamics", "dynamics_noise")):
        print(f"\n{title} Noise Degradation:")
        table = analysis[f"{fam}_degradation"]
        for level in sorted(table.keys()):
            row = table[level]
            print(f"  Noise std {level:.3f}:")
            print(f"    Success rate: {row['success_rate']:.1%}")
            print(f"    Degradation: {row['degradation']:.1%} ({row['degradation_percentage']:.1f}%)")
    print(rule)


# ------------------------------------------------------------------ the study on the device
def _tables_to_dicts(summ, keys, levels, first: int) -> Dict:
    """The sweep-shaped ``results`` (empty ``episodes`` lists) and the ``analysis`` dict of the
    ``len(keys)`` consecutive groups from ``first``, the first of them the baseline."""
    results: Dict[str, Any] = {"baseline": None, "observation_noise": {}, "dynamics_noise": {}, "combined_noise": {}}
    base = summ.level(first)
    analysis: Dict[str, Any] = {"baseline": {"success_rate": base["success_rate"],
                                             "mean_episode_length": base["mean_episode_length"]}}
    for fam in _FAMILIES:
        analysis[f"{fam}_degradation"] = {}
    for li, ((fam, key), (o, d)) in enumerate(zip(keys, levels)):
        r = {"episodes": [], "metrics": summ.metrics(first + li),
             "noise_levels": {"observation_noise_std": o, "dynamics_noise_std": d}}
        if fam == "baseline":
            results["baseline"] = r
        else:
            results[fam][key] = r
            analysis[f"{fam}_degradation"][key] = summ.level(first + li)
    return {"results": results, "analysis": analysis}


def run_robustness_study(policy, eval_config, observation_noise_levels: List[float],
                         dynamics_noise_levels: List[float], num_episodes: int = 20, seed: Optional[int] = None, *,
                         parallel: bool = True, policy_seeds: Optional[Sequence[int]] = None, device_seed: int = 0,
                         reward_type: str = "dense", max_episode_steps: int = 200,
                         timing: Optional[Dict] = None) -> Dict:
    """``RobustnessTester.run_robustness_sweep`` and ``analyze_robustness_results`` as one episode
    launch without a contact history and one ``dxrl_robustness_summarize`` (module docstring).

    The launch forms are the sweep's: ``parallel=False`` the exact order (one policy stream through
    all levels), ``parallel=True`` one lane per episode, with ``policy_seeds`` (one per episode,
    host reset and noise draws) or without (device draws under ``device_seed``).  Returns
    ``{"results": the sweep-shaped dict with empty "episodes" lists, "analysis": the analysis dict
    built from level_table, "summary": RobustnessSummary}``.

    ``eval_config`` may be a list of configs (up to ``MAX_CURRICULA``; ``parallel=True`` only): the
    launch carries every config's sweep, config c's level l is group ``c L + l`` with baseline
    ``c L``, and L pooled groups (all configs, level l, against the pooled baseline) follow;
    ``results`` / ``analysis`` are then the pooled ones and ``"per_config"`` lists the same pair per
    config.  This form always takes the reset and noise draws on the host, where a lane's episode
    does not depend on its lane index, so config c's slice equals the single-config study of that
    config with the same ``policy_seeds``; ``policy_seeds`` holds one seed per episode of one
    config's sweep (used for every config) or of the whole launch.  A policy that draws, run
    without ``policy_seeds``, takes its draws from the device stream of its lane."""
    from .evaluator import (EpisodeProgram, RobustnessTester, Segment, _exact_tape, _seeded_tapes, compiled_program)
    prog = compiled_program(policy)
    if prog is None:
        raise ValueError("a device robustness study needs a policy the episode kernel compiles")
    many = isinstance(eval_config, (list, tuple))
    configs = list(eval_config) if many else [eval_config]
    if many and not parallel:
        raise ValueError("a study over a list of configs is parallel=True only")
    if not configs:
        raise ValueError("no eval config")
    K = int(num_episodes)
    levels, keys = RobustnessTester.sweep_levels(observation_noise_levels, dynamics_noise_levels)
    L, C = len(levels), len(configs)
    rt = RobustnessTester(policy, configs[0], reward_type=reward_type, max_episode_steps=max_episode_steps)
    if not many:
        p = rt.levels_program(levels, K, seed, parallel, lane_per_level=prog.draws == 0)
    else:
        p = EpisodeProgram(configs, reward_type, max_episode_steps)
        for c in range(C):
            for o, d in levels:
                s = rt._level_segment(o, d, K, seed)
                for k, es in enumerate(s.episode_seeds):
                    p.add_lane([Segment(c, [es], o, d, noise_seed=None if seed is None else (seed, k))])
    level_rows = lambda c, li: np.arange((c * L + li) * K, (c * L + li + 1) * K)  # noqa: E731
    groups = [level_rows(c, li) for c in range(C) for li in range(L)]
    baseline = [c * L for c in range(C) for _ in range(L)]
    if many:
        groups += [np.concatenate([level_rows(c, li) for c in range(C)]) for li in range(L)]
        baseline += [C * L] * L
    kw: Dict[str, Any] = dict(groups=groups, summary="robustness", keep_history=False, timing=timing,
                              summary_options=dict(baseline_group=baseline, success_threshold=3, returns=False,
                                                   policy_used=not parallel))
    if not parallel:
        summ = p.run(prog, policy_tapes=_exact_tape(prog, p), **kw)
        prog.stream.commit(int(summ.policy_used[0]))  # the host stream is left where the sweep leaves it
    elif policy_seeds is not None:
        seeds = list(policy_seeds)
        if many and len(seeds) == L * K:
            seeds = seeds * C
        summ = p.run(prog, policy_tapes=_seeded_tapes(prog, p, seeds), **kw)
    elif many:
        summ = p.run(prog, host_resets=True, host_noise=True, device_seed=device_seed, **kw)
    else:
        summ = p.run(prog, host_resets=False, host_noise=False, device_seed=device_seed, **kw)
    out = _tables_to_dicts(summ, keys, levels, C * L if many else 0)
    if many:
        out["per_config"] = [_tables_to_dicts(summ, keys, levels, c * L) for c in range(C)]
    out["summary"] = summ
    return out


__all__ = ["analyze_robustness_results", "plot_robustness_results", "print_robustness_report",
           "run_robustness_study"]
