"""The component ablation of the policy-gradient trainer as a command.

``python -m dexterous_rl_manipulation_amd.pg_ablation [--config F | --config-name NAME] --iterations N
[--envs E --horizon T --max-steps S --seeds S ... --validate-every K --val-episodes E --out DIR
--host-summary --device D]``

Runs ``ablation.run_pg_component_study`` -- curriculum on / off x dense / sparse reward, every arm
over the seeds, every run validated on the same held-out objects -- prints the reference's
ablation report and the paired effects, and writes ``DIR/pg_component_ablation.json``: the
statistics dictionary and the whole ``StudyResult``.  Seeds, the scheduler's constants, the episode
step limit and the output directory default to the experiment configuration's
``component_ablation`` section (and its ``output_dir``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Any, Dict, List, Optional

JSON_NAME = "pg_component_ablation.json"


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m dexterous_rl_manipulation_amd.pg_ablation",
                                description="Component ablation (curriculum x reward) of the MLP actor-critic.")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--config", default=None, metavar="F", help="experiment configuration JSON file")
    g.add_argument("--config-name", default=None, metavar="NAME", help="predefined configuration (default, quick_test)")
    p.add_argument("--iterations", type=int, required=True, help="training iterations per run")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--horizon", type=int, default=200)
    p.add_argument("--max-steps", type=int, default=None, help="episode step limit (default: the configuration's)")
    p.add_argument("--seeds", type=int, nargs="+", default=None, help="default: the configuration's")
    p.add_argument("--validate-every", type=int, default=10, metavar="K",
                   help="held-out validation every K iterations and after the last (0: never)")
    p.add_argument("--val-episodes", type=int, default=5, metavar="E", help="validation episodes per held-out object")
    p.add_argument("--out", metavar="DIR", default=None, help="default: the configuration's output_dir")
    p.add_argument("--host-summary", action="store_true",
                   help="copy the runs' tables and reduce them with NumPy instead of on the device")
    p.add_argument("--device", default=None)
    a = p.parse_args(argv)
    if a.iterations < 1 or a.envs < 1 or a.horizon < 1 or a.validate_every < 0 or a.val_episodes < 1 or \
            (a.max_steps is not None and a.max_steps < 1):
        p.error("--iterations, --envs, --horizon, --max-steps and --val-episodes must be >= 1; --validate-every >= 0")
    return a


def study_arguments(a: argparse.Namespace) -> Dict[str, Any]:
    """``run_pg_component_study``'s keyword arguments (and ``output_dir``) from the command line
    and the experiment configuration."""
    from .experiments import load_config, load_named_config
    if a.config_name:
        exp = load_named_config(a.config_name)
    else:
        exp = load_config(a.config)
    ab = exp.component_ablation
    return {"iterations": a.iterations, "seeds": list(a.seeds if a.seeds is not None else ab.seeds),
            "curriculum_scheduler_config": ab.curriculum_scheduler, "num_envs": a.envs, "horizon": a.horizon,
            "max_steps": int(a.max_steps if a.max_steps is not None else ab.max_episode_steps),
            "validate_every": a.validate_every, "val_episodes": a.val_episodes,
            "device_summary": not a.host_summary, "device": a.device,
            "output_dir": a.out if a.out is not None else exp.output_dir}


def effect_lines(stats: Dict[str, Any]) -> List[str]:
    """The paired effects on the final success rate, one line per contrast."""
    lines = ["Paired effects on the final success rate (mean +/- standard error over the seeds):"]
    for name, e in stats.get("effects", {}).items():
        lines.append(f"  {name}: {e['mean']:+.3f} +/- {e['stderr']:.3f} ({e['pairs']} pairs)")
    return lines


def results_json(stats: Dict[str, Any], result) -> Dict[str, Any]:
    """pg_component_ablation.json: the statistics (NaN as a string, as in the study) and the study."""
    from .training_study import _encode

    def enc(x):
        return {k: enc(v) for k, v in x.items()} if isinstance(x, dict) else _encode(x)

    return {"statistics": enc(stats), "study": result.to_dict()}


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    kw = study_arguments(a)
    out_dir = kw.pop("output_dir")
    from . import ablation
    bar = "=" * 80
    print(bar)
    print("Component Ablation Study (policy-gradient trainer)")
    print(bar)
    print(f"  Iterations per run: {kw['iterations']}  ({kw['num_envs']} envs x {kw['horizon']} steps)")
    print(f"  Seeds: {kw['seeds']}")
    print(f"  Validation: every {kw['validate_every']} iterations, {kw['val_episodes']} episodes per object")
    stats, result = ablation.run_pg_component_study(return_study=True, **kw)
    ablation.print_ablation_report({}, stats)
    print("\n".join(effect_lines(stats)))
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, JSON_NAME)
    with open(path, "w") as f:
        json.dump(results_json(stats, result), f, indent=2, allow_nan=False)
    print(f"\nResults saved to: {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
