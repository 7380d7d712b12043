"""Statistical analysis of failure modes -- evaluation/failure_statistics.py:18-393, the
scripts evaluation/analyze_failures.py and evaluation/run_failure_logging.py, and the device
form of the whole study.

Host functions (``load_failure_logs`` ... ``generate_failure_report``): the reference's names,
signatures, dictionaries, printed text and files (``failure_distribution.png``,
``failure_correlations.png``, ``failure_analysis.json``), through the same NumPy calls on the
same lists.  ``python -m dexterous_rl_manipulation_amd.failure_statistics --log_file ...
--output_dir ...`` is ``analyze_failures.py``; ``run_failure_logging()`` is that example script.

``run_failure_study`` is the same analysis without per-episode data on the host: one episode
launch and one ``dxrl_failure_summarize`` (csrc/dxrl_failure_summary.hip) behind it classify
every episode by the taxonomy and reduce, per object group and failure mode, the sums the
dictionaries are made of; only those tables cross to the host.  Means of integers are S / n
(what np.mean returns), standard deviations come from the moments.  Modes appear in
``list(FailureMode)`` order (the host functions list them in order of first appearance).
"""
from __future__ import annotations

import json
import math
from collections import defaultdict
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

_BAR = "=" * 60


def _pyplot():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def load_failure_logs(filepath: str) -> List[Dict]:
    """failure_statistics.py:18-31: the ``episodes`` list of a FailureLogger JSON file."""
    with open(filepath, "r") as f:
        data = json.load(f)
    return data.get("episodes", [])


def _by_mode(episodes: List[Dict]) -> Dict[str, List[Dict]]:
    out: Dict[str, List[Dict]] = defaultdict(list)
    for ep in episodes:
        mode = ep.get("failure_mode")
        if mode:
            out[mode].append(ep)
    return out


def _final_contacts(ep: Dict):
    return ep.get("final_contacts", ep.get("num_contacts", 0))


def compute_failure_distribution(episodes: List[Dict]) -> Dict[str, Dict]:
    """failure_statistics.py:34-89."""
    if not episodes:
        return {}
    total = len(episodes)
    out = {}
    for mode, eps in _by_mode(episodes).items():
        lengths = [ep["episode_steps"] for ep in eps]
        final = [_final_contacts(ep) for ep in eps]
        sizes = [ep["object_properties"]["size"] for ep in eps]
        masses = [ep["object_properties"]["mass"] for ep in eps]
        frictions = [ep["object_properties"]["friction_coefficient"] for ep in eps]
        out[mode] = {
            "count": len(eps),
            "frequency": len(eps) / total if total > 0 else 0.0,
            "mean_episode_length": float(np.mean(lengths)) if lengths else 0.0,
            "std_episode_length": float(np.std(lengths)) if lengths else 0.0,
            "mean_final_contacts": float(np.mean(final)) if final else 0.0,
            "mean_object_size": float(np.mean(sizes)) if sizes else 0.0,
            "std_object_size": float(np.std(sizes)) if sizes else 0.0,
            "mean_object_mass": float(np.mean(masses)) if masses else 0.0,
            "std_object_mass": float(np.std(masses)) if masses else 0.0,
            "mean_friction": float(np.mean(frictions)) if frictions else 0.0,
            "std_friction": float(np.std(frictions)) if frictions else 0.0,
        }
    return out


def _spread(values, extremes: bool) -> Dict:
    out = {"mean": float(np.mean(values)), "std": float(np.std(values))}
    if extremes:
        out["min"], out["max"] = float(np.min(values)), float(np.max(values))
    return out


def compute_correlations(episodes: List[Dict]) -> Dict[str, Dict]:
    """failure_statistics.py:92-159: per mode with at least two episodes, the spread of the
    object properties, the episode length and the final contact count."""
    if not episodes:
        return {}
    out = {}
    for mode, eps in _by_mode(episodes).items():
        if len(eps) < 2:
            continue
        out[mode] = {
            "object_size": _spread([ep["object_properties"]["size"] for ep in eps], True),
            "object_mass": _spread([ep["object_properties"]["mass"] for ep in eps], True),
            "friction": _spread([ep["object_properties"]["friction_coefficient"] for ep in eps], True),
            "episode_length": _spread([ep["episode_steps"] for ep in eps], False),
            "contacts": _spread([_final_contacts(ep) for ep in eps], False),
        }
    return out


def plot_failure_distribution(episodes: List[Dict], output_path: str = "logs/failure_distribution.png") -> None:
    """failure_statistics.py:162-227: pie and bar chart of the mode counts, mean episode length
    (with its std) and mean final contacts per mode."""
    distribution = compute_failure_distribution(episodes)
    if not distribution:
        print("No failure episodes to plot")
        return
    plt = _pyplot()
    fig, axes = plt.subplots(2, 2, figsize=(14, 10))
    modes = list(distribution.keys())
    counts = [distribution[m]["count"] for m in modes]
    ax = axes[0, 0]
    ax.pie(counts, labels=modes, autopct="%1.1f%%", startangle=90)
    ax.set_title("Failure Mode Distribution (Pie Chart)")
    ax = axes[0, 1]
    bars = ax.bar(modes, counts, color="steelblue", alpha=0.7)
    ax.set_xlabel("Failure Mode")
    ax.set_ylabel("Count")
    ax.set_title("Failure Mode Distribution (Bar Chart)")
    ax.tick_params(axis="x", rotation=45)
    for bar in bars:
        h = bar.get_height()
        ax.text(bar.get_x() + bar.get_width() / 2.0, h, f"{int(h)}", ha="center", va="bottom")
    ax = axes[1, 0]
    ax.bar(modes, [distribution[m]["mean_episode_length"] for m in modes],
           yerr=[distribution[m]["std_episode_length"] for m in modes], color="coral", alpha=0.7, capsize=5)
    ax.set_xlabel("Failure Mode")
    ax.set_ylabel("Mean Episode Length (steps)")
    ax.set_title("Episode Length by Failure Mode")
    ax.tick_params(axis="x", rotation=45)
    ax = axes[1, 1]
    ax.bar(modes, [distribution[m]["mean_final_contacts"] for m in modes], color="lightgreen", alpha=0.7)
    ax.set_xlabel("Failure Mode")
    ax.set_ylabel("Mean Final Contacts")
    ax.set_title("Final Contacts by Failure Mode")
    ax.tick_params(axis="x", rotation=45)
    ax.set_ylim([0, 5])
    fig.tight_layout()
    fig.savefig(output_path, dpi=150)
    plt.close(fig)
    print(f"Failure distribution plot saved to {output_path}")


def plot_failure_correlations(episodes: List[Dict], output_path: str = "logs/failure_correlations.png") -> None:
    """failure_statistics.py:230-298: mean object size, mass and friction per mode (with their
    std) and a size / mass scatter coloured by mode."""
    correlations = compute_correlations(episodes)
    if not correlations:
        print("No correlation data to plot")
        return
    plt = _pyplot()
    fig, axes = plt.subplots(2, 2, figsize=(14, 10))
    modes = list(correlations.keys())
    panels = [(axes[0, 0], "object_size", "skyblue", "Mean Object Size (m)", "Object Size vs Failure Mode"),
              (axes[0, 1], "object_mass", "orange", "Mean Object Mass (kg)", "Object Mass vs Failure Mode"),
              (axes[1, 0], "friction", "lightcoral", "Mean Friction Coefficient", "Friction vs Failure Mode")]
    for ax, key, color, ylabel, title in panels:
        ax.bar(modes, [correlations[m][key]["mean"] for m in modes], yerr=[correlations[m][key]["std"] for m in modes],
               color=color, alpha=0.7, capsize=5)
        ax.set_xlabel("Failure Mode")
        ax.set_ylabel(ylabel)
        ax.set_title(title)
        ax.tick_params(axis="x", rotation=45)
    ax = axes[1, 1]
    colors = plt.cm.Set3(np.linspace(0, 1, len(modes)))
    for i, mode in enumerate(modes):
        eps = [ep for ep in episodes if ep.get("failure_mode") == mode]
        ax.scatter([ep["object_properties"]["size"] for ep in eps], [ep["object_properties"]["mass"] for ep in eps],
                   label=mode, alpha=0.6, color=colors[i], s=50)
    ax.set_xlabel("Object Size (m)")
    ax.set_ylabel("Object Mass (kg)")
    ax.set_title("Object Properties by Failure Mode")
    ax.legend(bbox_to_anchor=(1.05, 1), loc="upper left")
    ax.grid(True, alpha=0.3)
    fig.tight_layout()
    fig.savefig(output_path, dpi=150, bbox_inches="tight")
    plt.close(fig)
    print(f"Failure correlations plot saved to {output_path}")


def generate_failure_report(episodes: List[Dict], output_dir: str = "logs") -> Dict:
    """failure_statistics.py:301-393: distribution, correlations, both plots and
    ``failure_analysis.json`` under ``output_dir``, with the reference's printed report."""
    out_dir = Path(output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    print(_BAR)
    print("Failure Mode Statistical Analysis")
    print(_BAR)
    if not episodes:
        print("No failure episodes to analyze")
        return {}
    print("\n1. Computing failure distribution...")
    distribution = compute_failure_distribution(episodes)
    print(f"\n   Total failure episodes: {len(episodes)}")
    print(f"   Failure modes identified: {len(distribution)}")
    print("\n2. Failure Mode Distribution:")
    for mode, st in sorted(distribution.items(), key=lambda x: x[1]["count"], reverse=True):
        print(f"   {mode}:")
        print(f"     Count: {st['count']} ({st['frequency']:.1%})")
        print(f"     Mean episode length: {st['mean_episode_length']:.1f} ± {st['std_episode_length']:.1f}")
        print(f"     Mean final contacts: {st['mean_final_contacts']:.2f}")
    print("\n3. Computing correlations...")
    correlations = compute_correlations(episodes)
    print("\n4. Object Property Correlations:")
    for mode, c in correlations.items():
        print(f"   {mode}:")
        print(f"     Object size: {c['object_size']['mean']:.4f} ± {c['object_size']['std']:.4f}")
        print(f"     Object mass: {c['object_mass']['mean']:.4f} ± {c['object_mass']['std']:.4f}")
        print(f"     Friction: {c['friction']['mean']:.3f} ± {c['friction']['std']:.3f}")
    print("\n5. Generating visualizations...")
    plot_failure_distribution(episodes, str(out_dir / "failure_distribution.png"))
    plot_failure_correlations(episodes, str(out_dir / "failure_correlations.png"))
    results = {"total_episodes": len(episodes), "distribution": distribution, "correlations": correlations}
    results_path = out_dir / "failure_analysis.json"
    with open(results_path, "w") as f:
        json.dump(results, f, indent=2)
    print(f"\n6. Analysis results saved to {results_path}")
    print("\n" + _BAR)
    print("Key Insights")
    print(_BAR)
    if distribution:
        mode, st = max(distribution.items(), key=lambda x: x[1]["count"])
        print(f"\nMost common failure mode: {mode} ({st['frequency']:.1%})")
        print(f"  This suggests focusing improvement efforts on: {mode}")
        if correlations:
            print("\nProperty correlations:")
            for mode, c in correlations.items():
                print(f"  {mode}:")
                print(f"    Tends to occur with: size={c['object_size']['mean']:.4f}m, "
                      f"mass={c['object_mass']['mean']:.4f}kg, friction={c['friction']['mean']:.3f}")
    print(_BAR)
    return results


# ------------------------------------------------------------------ the study from device tables
_PROP_KEYS = (("object_size", "mean_object_size", "std_object_size"),
              ("object_mass", "mean_object_mass", "std_object_mass"),
              ("friction", "mean_friction", "std_friction"))


def _int_std(n: int, s1: int, s2: int) -> float:
    """np.std of integers from their exact sums: sqrt((n S2 - S1^2) / n^2)."""
    return math.sqrt((n * s2 - s1 * s1) / (n * n))


def tables_to_dicts(mode_stats, group_totals, mode_props, g: int) -> Dict[str, Dict]:
    """``statistics`` (analyze_failure_modes' keys, no episode lists), ``distribution`` and
    ``correlations`` (over the failed episodes) of group ``g`` of a failure summary's tables."""
    from .failures import FailureMode
    names = [m.value for m in FailureMode]
    total, ok = int(group_totals[g, 0]), int(group_totals[g, 1])
    counts = {names[k]: int(mode_stats[g, k, 0]) for k in range(len(names))}
    failed = total - ok
    statistics: Dict[str, Any] = {
        "total_episodes": total, "successful_episodes": ok, "failed_episodes": failed,
        "success_rate": ok / total if total > 0 else 0.0, "failure_counts": counts,
        "failure_frequencies": {k: (v / total if total > 0 else 0.0) for k, v in counts.items()},
        "detailed_analysis": {}}
    distribution, correlations = {}, {}
    for k, name in enumerate(names):
        n, s_len, s_len2, s_c, s_c2 = (int(x) for x in mode_stats[g, k, :5])
        if n == 0:
            continue
        statistics["detailed_analysis"][name] = {"count": n, "mean_episode_length": float(s_len / n),
                                                 "mean_contacts": float(s_c / n)}
        d = {"count": n, "frequency": n / failed if failed > 0 else 0.0, "mean_episode_length": s_len / n,
             "std_episode_length": _int_std(n, s_len, s_len2), "mean_final_contacts": s_c / n}
        c = {}
        for q, (key, mean_key, std_key) in enumerate(_PROP_KEYS):
            pn, mean, m2, lo, hi = (float(x) for x in mode_props[g, k, q])
            std = math.sqrt(m2 / pn)
            d[mean_key], d[std_key] = mean, std
            c[key] = {"mean": mean, "std": std, "min": lo, "max": hi}
        distribution[name] = d
        if n >= 2:
            c["episode_length"] = {"mean": s_len / n, "std": _int_std(n, s_len, s_len2)}
            c["contacts"] = {"mean": s_c / n, "std": _int_std(n, s_c, s_c2)}
            correlations[name] = c
    return {"statistics": statistics, "distribution": distribution, "correlations": correlations}


def host_failure_study(episodes: List[Dict], classify_max_steps: int = 200, success_threshold: int = 3) -> Dict:
    """The host pipeline of the same study on episode dictionaries (``evaluate_heldout_set``'s
    ``all_episodes``): ``analyze_failure_modes`` classifies every episode in a Python loop, the
    failed ones take the logged form (``object_properties``) and go through
    ``compute_failure_distribution`` / ``compute_correlations``."""
    from .failure_analysis import analyze_failure_modes
    statistics = analyze_failure_modes(episodes, max_steps=classify_max_steps, success_threshold=success_threshold)
    failed = [dict(ep, object_properties={"size": ep["object_size"], "mass": ep["object_mass"],
                                          "friction_coefficient": ep["friction_coefficient"]})
              for ep in episodes if ep.get("failure_mode")]
    del statistics["classified_episodes"]
    for v in statistics["detailed_analysis"].values():
        del v["episodes"]
    return {"statistics": statistics, "distribution": compute_failure_distribution(failed),
            "correlations": compute_correlations(failed)}


def run_failure_study(policy, heldout_set, num_episodes_per_object: int = 5, seed: Optional[int] = None, *,
                      max_episode_steps: int = 200, classify_max_steps: int = 200, parallel: bool = True,
                      policy_seeds: Optional[Sequence[int]] = None, device_seed: int = 0, keep_history: bool = True,
                      per_object: bool = True, success_threshold: int = 3, timing: Optional[Dict] = None,
                      reward_type: str = "dense", device=None) -> Dict:
    """The failure-mode study of a held-out evaluation on the device (module docstring):
    ``Evaluator.failure_study`` -- one episode launch, one ``dxrl_failure_summarize`` -- and the
    reference's dictionaries finished on the host from its tables.

    Returns ``statistics`` / ``distribution`` / ``correlations`` over all episodes,
    ``per_object[o]`` with the same three per object group (``per_object=True``), ``tie_rows``
    (episodes where np.var's rounding decides a rule: settled with ``FailureClassifier.classify``
    on those rows when a history is kept, decided by the exact integer comparison with
    ``keep_history=False``) and ``bytes_to_host``.  ``classify_max_steps`` is the classifier's
    timeout bound: an episode of this env fails only by running out of steps, so with the loop
    bound itself every failure is a timeout; the other modes appear under a larger bound, as
    ``run_failure_logging`` classifies at the default 200.  Object properties the device draws
    (a curriculum with ranges, ``parallel=True`` without ``policy_seeds``) are unknown to the host:
    ``ValueError``."""
    from .evaluator import Evaluator
    ev = Evaluator(policy=policy, heldout_set=heldout_set, reward_type=reward_type,
                   max_episode_steps=max_episode_steps, device=device)
    summ = ev.failure_study(num_episodes_per_object, seed, classify_max_steps=classify_max_steps, parallel=parallel,
                            policy_seeds=policy_seeds, device_seed=device_seed, keep_history=keep_history,
                            per_object=per_object, success_threshold=success_threshold, timing=timing)
    G = len(summ.group_totals)
    out = tables_to_dicts(summ.mode_stats, summ.group_totals, summ.mode_props, G - 1)
    out["per_object"] = {o: tables_to_dicts(summ.mode_stats, summ.group_totals, summ.mode_props, o)
                         for o in range(G - 1)} if per_object else {}
    out["tie_rows"] = [int(e) for e in summ.tie_rows]
    out["bytes_to_host"] = int(summ.host_bytes)
    out["summary"] = summ
    return out


# ------------------------------------------------------------------ scripts
def run_failure_logging(num_heldout_objects: int = 10, num_episodes_per_object: int = 5, seed: int = 42,
                        log_dir: str = "logs/failures", max_episode_steps: int = 200, device=None) -> Dict:
    """evaluation/run_failure_logging.py: RandomPolicy on held-out objects of the hard
    curriculum with a FailureLogger, the logged failures analysed at the default bound and saved
    as ``failure_episodes.json``."""
    from . import envs, evaluation, policies
    from .experiments import CurriculumConfig
    from .failure_analysis import analyze_failure_modes, print_failure_statistics
    print(_BAR)
    print("Failure Logging Example")
    print(_BAR)
    print("\n1. Setting up evaluation...")
    train_config = CurriculumConfig.hard()
    heldout_set = evaluation.HeldOutObjectSet(train_config, num_heldout_objects=num_heldout_objects, seed=42)
    env = envs.DexterousManipulationEnv(curriculum_config=train_config)
    policy = policies.RandomPolicy(env.action_space, seed=42)
    env.close()
    print("2. Creating failure logger...")
    logger = evaluation.FailureLogger(log_dir=log_dir, save_full_trajectories=True, success_threshold=3)
    print(f"   Logger will save to: {logger.log_dir}")
    print(f"   Full trajectories: {logger.save_full_trajectories}")
    print("3. Creating evaluator with failure logger...")
    evaluator = evaluation.Evaluator(policy=policy, heldout_set=heldout_set, reward_type="dense",
                                     max_episode_steps=max_episode_steps, failure_logger=logger, device=device)
    print("   Evaluator configured to log failures automatically")
    print("\n4. Running evaluation...")
    print("   (Failures will be automatically logged)")
    evaluator.evaluate_heldout_set(num_episodes_per_object=num_episodes_per_object, seed=seed)
    print("\n5. Analyzing logged failures...")
    num_logged = len(logger.logged_episodes)
    print(f"   Logged {num_logged} failure episodes")
    analysis = None
    if num_logged > 0:
        stats = logger.get_statistics()
        print("\n   Failure statistics:")
        print(f"     Total episodes: {stats['total_episodes']}")
        print("     Failure mode distribution:")
        for mode, count in stats["failure_mode_counts"].items():
            print(f"       {mode}: {count}")
        analysis = analyze_failure_modes([
            {"success": False, "episode_steps": ep["episode_steps"], "num_contacts": ep["num_contacts"],
             "final_contacts": ep["final_contacts"], "contact_history": ep["contact_history"]}
            for ep in logger.logged_episodes])
        print_failure_statistics(analysis)
        example = logger.logged_episodes[0]
        print("\n6. Example logged episode structure:")
        print(f"   Episode ID: {example['episode_id']}")
        print(f"   Failure mode: {example['failure_mode']}")
        print(f"   Episode steps: {example['episode_steps']}")
        print(f"   States recorded: {len(example.get('states', []))}")
        print(f"   Actions recorded: {len(example.get('actions', []))}")
        print(f"   Contacts recorded: {len(example.get('contact_history', []))}")
        print(f"   Metadata keys: {list(example.get('metadata', {}).keys())}")
    else:
        print("\n   [NOTE] No failures logged")
        print("          All episodes succeeded (or evaluation was too short)")
        print("          Try with harder configuration or more episodes")
    print("\n7. Saving logged failures...")
    log_path = logger.save("failure_episodes.json")
    print(f"   Saved to: {log_path}")
    print("\n8. Reproducibility information:")
    if num_logged > 0:
        metadata = logger.logged_episodes[0].get("metadata", {})
        print("   Example episode can be reproduced with:")
        print(f"     Seed: {metadata.get('seed')}")
        print(f"     Object size: {metadata.get('object_size')}")
        print(f"     Object mass: {metadata.get('object_mass')}")
        print(f"     Friction: {metadata.get('friction_coefficient')}")
        print("   All states, actions, and contacts are saved for offline analysis")
    print("\n" + _BAR)
    print("Failure Logging Complete")
    print(_BAR)
    return {"logger": logger, "analysis": analysis, "log_path": log_path}


def main(argv: Optional[Sequence[str]] = None):
    """evaluation/analyze_failures.py."""
    import argparse
    parser = argparse.ArgumentParser(description="Analyze failure episodes")
    parser.add_argument("--log_file", type=str, default="logs/failures/failure_episodes.json",
                        help="Path to failure log JSON file")
    parser.add_argument("--output_dir", type=str, default="logs", help="Directory to save analysis results")
    args = parser.parse_args(argv)
    print(f"Loading failure episodes from {args.log_file}...")
    try:
        episodes = load_failure_logs(args.log_file)
        print(f"Loaded {len(episodes)} failure episodes")
    except FileNotFoundError:
        print(f"Error: File not found: {args.log_file}")
        print("Please run evaluation with failure logging first.")
        return
    if not episodes:
        print("No failure episodes found in log file")
        return
    generate_failure_report(episodes, output_dir=args.output_dir)
    print("\nAnalysis complete!")
    print(f"Results saved to {args.output_dir}/")
    print("  - failure_distribution.png")
    print("  - failure_correlations.png")
    print("  - failure_analysis.json")


__all__ = ["load_failure_logs", "compute_failure_distribution", "compute_correlations", "plot_failure_distribution",
           "plot_failure_correlations", "generate_failure_report", "run_failure_study", "host_failure_study",
           "tables_to_dicts", "run_failure_logging"]

if __name__ == "__main__":
    main()
