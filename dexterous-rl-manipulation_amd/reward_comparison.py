"""Sparse against dense reward -- training/reward_comparison.py on the policy-gradient trainer.

The reference trains a ``SimpleLearner`` for ``num_episodes`` episodes under each reward and
compares mean reward, final success rate and the first window of episodes whose mean reward
exceeds 0.5.  Its own copy cannot run (``run_training_comparison`` reads ``stats["total_reward"]``,
a key ``run_training_episode`` does not return: SURVEY quirk 8).  Here each arm is one
``PGTrainer.fit`` of the MLP actor-critic on ``num_envs`` envs with that reward, and the returned
dictionaries keep the reference's keys with one entry per logged ITERATION where the reference has
one per episode: ``episode_rewards`` is the log's ``mean_return`` column (the mean return of the
episodes the iteration finished), ``episode_steps`` its ``mean_length``, ``success_rates`` its
``success_rate``; ``mean_step_rewards`` (added) is its ``mean_step_reward``, the mean reward per
env step.

The two rewards are on different scales (an episode's dense return grows with its length, a sparse
one is at most 1), so ``convergence_step`` -- the reference's yardstick, a threshold on the return
-- does not mean the same thing in both arms.  ``success_convergence_step`` applies the same
window rule to ``success_rate`` (>= 3 contacts, the evaluators' rule) and does.

The arms run one after the other on the trainer's stream.

``python -m dexterous_rl_manipulation_amd.reward_comparison --iterations N [--envs E --horizon T
--max-steps S --out DIR --validate-every K --curriculum NAME]``
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Any, Dict, List, Optional

import numpy as np

_BAR = "=" * 60
ARMS = ("sparse", "dense")  # the reference's order (reward_comparison.py:159-165)
# the keys of reward_comparison.json per arm: the reference's five (reward_comparison.py:190-205) ...
REFERENCE_JSON_KEYS = ("mean_reward", "std_reward", "final_success_rate", "convergence_step", "episode_rewards")
# ... and what this build adds
ADDED_JSON_KEYS = ("episode_steps", "success_rates", "mean_step_rewards", "success_convergence_step", "iterations",
                   "reward_type")
VALIDATION_JSON_KEYS = ("validation_iterations", "validation_success_rates")


def window_convergence(values, window: int, threshold: float) -> Optional[int]:
    """reward_comparison.py:121-124 over a whole series: the index of the first entry of the first
    window of `window` consecutive entries whose mean is strictly above `threshold`, or None (a
    window holding a NaN -- an iteration that finished no episode -- has a NaN mean and does not
    qualify, as on the device)."""
    values = np.asarray(values, dtype=np.float64)
    window = int(window)
    for last in range(window - 1, len(values)):
        if np.mean(values[last - window + 1:last + 1]) > threshold:
            return last - window + 1
    return None


def comparison_from_log(log, reward_type: str, convergence_threshold: float = 0.5,
                        convergence_window: int = 10) -> Dict[str, Any]:
    """The reference's result dictionary (reward_comparison.py:128-136) from a ``TrainingLog``.

    ``convergence_step`` is ``log.convergence_iteration``: the ``iteration`` value of the first
    row of the first window whose mean ``mean_return`` exceeded the threshold, i.e. the reference's
    ``episode - window + 1`` with iterations for episodes (a fresh run's row r is iteration r).
    ``mean_reward`` / ``std_reward`` are over the rows that finished at least one episode (the
    others carry NaN); ``final_success_rate`` is the mean of the last 10 rows, or of all rows when
    there are fewer (NaN when one of them finished no episode)."""
    rewards, steps, rates = (np.array(log[c], dtype=np.float64) for c in ("mean_return", "mean_length", "success_rate"))
    finished = np.asarray(log["episodes"]) >= 1
    got = rewards[finished]
    tail = rates[-10:] if len(rates) >= 10 else rates
    start = int(log["iteration"][0]) if len(log) else 0
    by_success = window_convergence(rates, convergence_window, convergence_threshold)
    return {
        "reward_type": reward_type,
        "episode_rewards": rewards.tolist(),
        "episode_steps": steps.tolist(),
        "success_rates": rates.tolist(),
        "mean_step_rewards": np.array(log["mean_step_reward"], dtype=np.float64).tolist(),
        "convergence_step": log.convergence_iteration,
        "mean_reward": float(np.mean(got)) if got.size else float("nan"),
        "std_reward": float(np.std(got)) if got.size else float("nan"),
        "final_success_rate": float(np.mean(tail)) if tail.size else float("nan"),
        "success_convergence_step": None if by_success is None else start + by_success,
        "log": log,
    }


def run_training_comparison(reward_type: str, num_iterations: int = 100, *, num_envs: int = 4096, horizon: int = 200,
                            max_steps: int = 200, seed: int = 42, curriculum_config=None,
                            convergence_threshold: float = 0.5, convergence_window: int = 10, heldout_set=None,
                            validate_every: int = 0, val_episodes: int = 5, val_seed: int = 0, device=None,
                            **trainer_kw) -> Dict[str, Any]:
    """One arm: ``fit(num_iterations, converge=("mean_return", window, threshold))`` of a fresh
    ``PGTrainer`` on ``num_envs`` envs with ``reward_type`` ("sparse" or "dense"), env and trainer
    seeded with ``seed``; ``trainer_kw`` goes to ``TrainerConfig``.  Returns ``comparison_from_log``'s
    dictionary.  With ``heldout_set`` and ``validate_every`` > 0 the run validates on that set every
    ``validate_every`` iterations (``val_episodes`` per object, reset seed ``val_seed`` -- the same
    plan in both arms) and the dictionary also carries ``validation_iterations`` and
    ``validation_success_rates``, the held-out success-rate curve."""
    from .envs import VecEnv
    from .trainer import PGTrainer, TrainerConfig
    if reward_type not in ARMS:
        raise ValueError(f"reward_type must be 'sparse' or 'dense', got {reward_type!r}")
    env = VecEnv(num_envs, curriculum_config=curriculum_config, reward_type=reward_type, max_episode_steps=max_steps,
                 seed=seed, device=device)
    tr = PGTrainer(env, TrainerConfig(horizon=horizon, seed=seed, max_steps=max_steps, **trainer_kw))
    env.reset(write_obs=False)
    kw = {}
    if heldout_set is not None and validate_every:
        plan = tr.validation_plan(heldout_set, episodes_per_object=val_episodes, seed=val_seed, max_steps=max_steps)
        kw = dict(validation=plan, validate_every=int(validate_every))
    log = tr.fit(num_iterations, converge=("mean_return", int(convergence_window), float(convergence_threshold)), **kw)
    out = comparison_from_log(log, reward_type, convergence_threshold, convergence_window)
    if log.validation is not None:
        out["validation_iterations"] = [int(x) for x in log.validation["iteration"]]
        out["validation_success_rates"] = np.asarray(log.validation["success_rate"], dtype=np.float64).tolist()
    return out


def report_lines(sparse: Dict[str, Any], dense: Dict[str, Any]) -> List[str]:
    """The reference's printed comparison (reward_comparison.py:168-185), plus the convergence of
    the success rate; the improvement line only when both arms converged."""
    lines = ["", _BAR, "Results Comparison", _BAR]
    for title, r in (("Sparse Reward:", sparse), ("Dense Reward:", dense)):
        lines += ["", title,
                  f"  Mean reward: {r['mean_reward']:.3f} ± {r['std_reward']:.3f}",
                  f"  Final success rate: {r['final_success_rate']:.3f}",
                  f"  Convergence step: {r['convergence_step']}",
                  f"  Success-rate convergence step: {r['success_convergence_step']}"]
    s, d = sparse["convergence_step"], dense["convergence_step"]
    if s is not None and d is not None:
        # (sparse - dense) / sparse, as the reference, which divides by zero when the sparse arm
        # converged in its first window
        if s:
            lines += ["", f"Convergence improvement: {(s - d) / s * 100:.1f}% faster with dense rewards"]
        else:
            lines += ["", "Convergence improvement: n/a (the sparse arm converged at step 0)"]
    return lines


def _json_number(x):
    """NaN as None: the file stays standard JSON."""
    x = float(x)
    return x if np.isfinite(x) else None


def results_json(sparse: Dict[str, Any], dense: Dict[str, Any]) -> Dict[str, Any]:
    """reward_comparison.json: per arm the reference's keys, the added series and, after a
    validated run, the held-out curve."""
    out = {}
    for name, r in (("sparse", sparse), ("dense", dense)):
        arm = {"mean_reward": _json_number(r["mean_reward"]), "std_reward": _json_number(r["std_reward"]),
               "final_success_rate": _json_number(r["final_success_rate"]),
               "convergence_step": r["convergence_step"],
               "episode_rewards": [_json_number(x) for x in r["episode_rewards"]],
               "episode_steps": [_json_number(x) for x in r["episode_steps"]],
               "success_rates": [_json_number(x) for x in r["success_rates"]],
               "mean_step_rewards": [_json_number(x) for x in r["mean_step_rewards"]],
               "success_convergence_step": r["success_convergence_step"],
               "iterations": len(r["episode_rewards"]), "reward_type": r["reward_type"]}
        if "validation_success_rates" in r:
            arm["validation_iterations"] = list(r["validation_iterations"])
            arm["validation_success_rates"] = [_json_number(x) for x in r["validation_success_rates"]]
        out[name] = arm
    return out


def compare_rewards(num_iterations: int = 100, max_steps: int = 200, output_dir: str = "logs", **kw) -> Dict[str, Any]:
    """reward_comparison.py:139-214: the sparse arm, then the dense arm, both from seed 42 (``kw``
    goes to ``run_training_comparison``); prints the report, writes
    ``output_dir/reward_comparison.json`` and returns that dictionary."""
    kw.setdefault("seed", 42)
    print(_BAR)
    print("Reward Shaping Comparison: Sparse vs Dense")
    print(_BAR)
    print("\nRunning sparse reward training...")
    sparse = run_training_comparison("sparse", num_iterations, max_steps=max_steps, **kw)
    print("Running dense reward training...")
    dense = run_training_comparison("dense", num_iterations, max_steps=max_steps, **kw)
    print("\n".join(report_lines(sparse, dense)))
    os.makedirs(output_dir, exist_ok=True)
    results = results_json(sparse, dense)
    path = os.path.join(output_dir, "reward_comparison.json")
    with open(path, "w") as f:
        json.dump(results, f, indent=2, allow_nan=False)
    print(f"\nResults saved to {path}")
    print(_BAR)
    return results


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m dexterous_rl_manipulation_amd.reward_comparison",
                                description="Train the MLP actor-critic under the sparse and the dense reward "
                                            "and compare the two runs.")
    p.add_argument("--iterations", type=int, required=True, help="training iterations per arm")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--horizon", type=int, default=200)
    p.add_argument("--max-steps", type=int, default=200, help="episode step limit")
    p.add_argument("--out", metavar="DIR", default="logs")
    p.add_argument("--validate-every", type=int, default=0, metavar="K",
                   help="validate both arms on the same held-out objects every K iterations (0: never)")
    p.add_argument("--curriculum", default=None, metavar="NAME",
                   choices=("easy", "medium", "hard", "variable", "default"),
                   help="a CurriculumConfig preset (easy, medium, hard, variable, default); default: the env's own "
                        "object, as the reference's comparison")
    p.add_argument("--device", default=None)
    a = p.parse_args(argv)
    if a.iterations < 0 or a.envs < 1 or a.horizon < 1 or a.max_steps < 1 or a.validate_every < 0:
        p.error("--iterations and --validate-every must be >= 0; --envs, --horizon and --max-steps >= 1")
    return a


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    from .experiments import CurriculumConfig
    kw: Dict[str, Any] = dict(num_envs=a.envs, horizon=a.horizon, device=a.device)
    if a.curriculum is not None:
        kw["curriculum_config"] = CurriculumConfig.named(a.curriculum)
    if a.validate_every:
        from .evaluation import HeldOutObjectSet
        kw.update(heldout_set=HeldOutObjectSet(kw.get("curriculum_config") or CurriculumConfig()),
                  validate_every=a.validate_every)
    compare_rewards(a.iterations, a.max_steps, a.out, **kw)
    return 0


__all__ = ["run_training_comparison", "compare_rewards", "comparison_from_log", "window_convergence", "report_lines",
           "results_json"]

if __name__ == "__main__":
    sys.exit(main())
