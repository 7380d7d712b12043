"""Golden fixture for the curriculum-ablation drivers.

Run on the CPU where gen_golden.py's conditions hold (the reference checkout it names is
present), with ``python3 -B``, like gen_eval_golden.py.

Imports the reference read-only (through gen_golden's gymnasium stand-in) and
records what evaluation/curriculum_ablation.py returns:

* ``train_with_curriculum`` / ``train_without_curriculum(use_hard=True)``
  (:25-134) for seeds 42 and 43, 40 episodes, every returned list, the
  scheduler statistics, ``compute_convergence_metrics`` (:137-203) of each and
  two np.random values drawn afterwards;
* one run in which the reference's scheduler itself progresses:
  ``component_ablation.train_with_config`` with a threshold-0.0 scheduler
  (the all-False success window passes ``0.0 >= 0.0``), dense and sparse --
  the row switch, the numpy.float64 friction of an interpolated level and the
  sticky object position;
* ``run_ablation_study(num_episodes=40, num_runs=2)``'s result dictionary.

The reference seeds every env stream from OS entropy (``env.reset()`` without a
seed); for capture the stand-in's lazy seeding is pinned to the recorded
``env_seed`` values, which the build's drivers take as arguments.

Output (committed): tests/golden/curriculum_golden.json.
"""
import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the stand-in, puts the reference on sys.path)

from evaluation import curriculum_ablation as CA  # noqa: E402
from evaluation.component_ablation import AblationConfig, train_with_config  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NUM_EPISODES = 40
RUNS = [(42, 2101, 2201), (43, 2102, 2202)]  # learner seed, env seed with / without curriculum
PROGRESSING = dict(initial_difficulty="easy", target_difficulty="hard", success_rate_threshold=0.0, window_size=4,
                   min_episodes_before_progression=6, progression_steps=3)
STUDY_ENV_SEEDS = [3001, 3002, 3003, 3004]  # in the order run_ablation_study builds its envs


def jsonable(x):
    if isinstance(x, dict):
        return {str(k): jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if isinstance(x, (np.bool_, bool)):
        return bool(x)
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    if isinstance(x, np.ndarray):
        return jsonable(x.tolist())
    return x


class pinned_env_seeds:
    """Entropy-seeded generators (``_pcg(None)``) take the given seeds, in order."""

    def __init__(self, seeds):
        self.seeds, self.used = list(seeds), 0

    def __enter__(self):
        self.orig = G._pcg

        def pcg(s):
            if s is not None:
                return self.orig(s)
            self.used += 1
            return self.orig(self.seeds[self.used - 1])

        G._pcg = pcg
        return self

    def __exit__(self, *exc):
        G._pcg = self.orig


def gen_runs():
    out = []
    for seed, es_with, es_without in RUNS:
        with pinned_env_seeds([es_with]) as p:
            w = CA.train_with_curriculum(num_episodes=NUM_EPISODES, seed=seed)
            after_w = np.random.standard_normal(2)
            assert p.used == 1
        with pinned_env_seeds([es_without]) as p:
            wo = CA.train_without_curriculum(num_episodes=NUM_EPISODES, seed=seed, use_hard=True)
            after_wo = np.random.standard_normal(2)
            assert p.used == 1
        out.append(dict(seed=seed, env_seed_with=es_with, env_seed_without=es_without, with_curriculum=w,
                        without_curriculum=wo, np_random_after_with=after_w, np_random_after_without=after_wo,
                        metrics_with=CA.compute_convergence_metrics(w["episode_rewards"], w["success_rates"]),
                        metrics_without=CA.compute_convergence_metrics(wo["episode_rewards"], wo["success_rates"])))
    return out


def gen_progressing():
    out = []
    for dense, env_seed in [(True, 1101), (False, 1102)]:
        with pinned_env_seeds([env_seed]) as p:
            r = train_with_config(AblationConfig(True, dense), num_episodes=30, max_episode_steps=50, seed=42,
                                  curriculum_scheduler_config=types.SimpleNamespace(**PROGRESSING))
            after = np.random.standard_normal(2)
            assert p.used == 1
        out.append(dict(use_dense_reward=dense, seed=42, env_seed=env_seed, num_episodes=30, max_episode_steps=50,
                        scheduler=PROGRESSING, result=r.to_dict(), np_random_after=after))
    return out


def gen_study():
    with tempfile.TemporaryDirectory() as d, pinned_env_seeds(STUDY_ENV_SEEDS) as p:
        buf = io.StringIO()
        with redirect_stdout(buf):
            res = CA.run_ablation_study(num_episodes=NUM_EPISODES, num_runs=2, output_dir=d)
        saved = json.load(open(os.path.join(d, "curriculum_ablation.json")))
        assert p.used == len(STUDY_ENV_SEEDS)
    text = buf.getvalue().replace(d, "<output_dir>")
    return dict(num_episodes=NUM_EPISODES, num_runs=2, env_seeds_with=STUDY_ENV_SEEDS[:2],
                env_seeds_without=STUDY_ENV_SEEDS[2:], result=res, saved=saved, report=text)


def main():
    meta = {"generator": "tests/golden/gen_curriculum_golden.py", "numpy": np.__version__,
            "num_episodes": NUM_EPISODES, "runs": gen_runs(), "progressing": gen_progressing(),
            "study": gen_study()}
    path = os.path.join(OUT, "curriculum_golden.json")
    with open(path, "w") as f:
        json.dump(jsonable(meta), f, indent=None, separators=(",", ":"))
    print("wrote", path)


if __name__ == "__main__":
    main()
