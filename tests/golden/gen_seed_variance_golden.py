"""Golden fixture for the seed-variance driver.

Run on the CPU where gen_golden.py's conditions hold (the reference checkout it names is
present), with ``python3 -B`` and ``MPLBACKEND=Agg``, like gen_curriculum_golden.py.

Imports the reference read-only (through gen_golden's gymnasium stand-in) and records what
evaluation/seed_variance.py's ``analyze_seed_variance`` (:335-446) returns for three frozen
policies -- RandomPolicy (space seed 42), HeuristicPolicy and a SimpleLearner with a non-zero
``mean_action`` -- each with seeds [42, 123, 456], 4 held-out objects, 2 episodes per object and
``max_episode_steps=40``: the returned dict, the saved JSON, the captured report text (the
output directory replaced by ``<output_dir>``) and two values drawn from the policy's stream
afterwards.

Output (committed): tests/golden/seed_variance_golden.json.
"""
import io
import json
import os
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the stand-in, puts the reference on sys.path)
from gen_curriculum_golden import jsonable  # noqa: E402

from envs import DexterousManipulationEnv  # noqa: E402
from evaluation.heldout_objects import HeldOutObjectSet  # noqa: E402
from evaluation.seed_variance import analyze_seed_variance  # noqa: E402
from policies.heuristic_policy import HeuristicPolicy  # noqa: E402
from policies.random_policy import RandomPolicy  # noqa: E402
from policies.simple_learner import SimpleLearner  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEEDS = [42, 123, 456]
HELDOUT = ("medium", 4, 42)
K, MAX_STEPS, CV = 2, 40, 0.2
MEAN = [-0.3, -0.2, -0.1, 0.1, 0.2, 0.3, -0.4, -0.4, 0.0, 0.25, -0.25, 0.1, -0.1, 0.05, -0.05]
CASES = [dict(policy="random", space_seed=42, np_seed=0), dict(policy="heuristic", np_seed=5),
         dict(policy="simple", np_seed=11)]


def make_policy(c):
    space = DexterousManipulationEnv().action_space
    if c["policy"] == "simple":
        p = SimpleLearner(space)
        p.mean_action = np.asarray(MEAN, dtype=np.float32)
        return p
    if c["policy"] == "heuristic":
        return HeuristicPolicy(space)
    space.seed(c["space_seed"])
    return RandomPolicy(space, seed=42)


def gen(c):
    h = HeldOutObjectSet(G.make_cfg(HELDOUT[0]), num_heldout_objects=HELDOUT[1], seed=HELDOUT[2])
    pol = make_policy(c)
    np.random.seed(c["np_seed"])
    buf = io.StringIO()
    with tempfile.TemporaryDirectory() as d:
        with redirect_stdout(buf):
            res = analyze_seed_variance(pol, h, seeds=list(SEEDS), num_episodes_per_object=K, reward_type="dense",
                                        max_episode_steps=MAX_STEPS, output_dir=d, max_cv_threshold=CV)
        saved = json.load(open(os.path.join(d, "seed_variance_analysis.json")))
        assert os.path.getsize(os.path.join(d, "seed_variance.png")) > 0
        text = buf.getvalue().replace(d, "<output_dir>")
    after = pol.action_space.np_random.random(2) if c["policy"] == "random" else np.random.standard_normal(2)
    return dict(c, result=res, saved=saved, report=text, stream_after=after)


def main():
    meta = {"generator": "tests/golden/gen_seed_variance_golden.py", "numpy": np.__version__, "seeds": SEEDS,
            "heldout": list(HELDOUT), "K": K, "max_steps": MAX_STEPS, "max_cv_threshold": CV, "mean": MEAN,
            "cases": [gen(c) for c in CASES]}
    path = os.path.join(OUT, "seed_variance_golden.json")
    with open(path, "w") as f:
        json.dump(jsonable(meta), f, indent=None, separators=(",", ":"))
    print("wrote", path)


if __name__ == "__main__":
    main()
