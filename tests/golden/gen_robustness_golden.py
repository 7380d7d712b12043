"""Golden fixture for the robustness analysis (evaluation/robustness_analysis.py).

Run ONLY in the build container, after gen_golden.py's conditions hold:

    cd /tmp && python3 -B <repository>/tests/golden/gen_robustness_golden.py

Imports the reference read-only (through gen_golden's gymnasium stand-in) and records what its
``analyze_robustness_results`` returns and ``print_robustness_report`` prints on two inputs:

(a) a hand-written results dict: baseline success 0.0 (the ``else 0.0`` branch of the
    percentage) in one variant and 0.6 in the other, a level better than the baseline (negative
    degradation), level keys out of order, an empty ``combined_noise``;
(b) a real ``RobustnessTester.run_robustness_sweep`` of the reference: medium curriculum, loop
    bound 20, 6 episodes per level, observation levels [0.05, 0.5], dynamics levels [0.3, 1.0],
    seed 11, RandomPolicy(seed=42) on an action space seeded with 7 (at bound 12 every level of
    this sweep has the baseline's success rate; at 20 some levels do better than it).  Asserted
    here: no variance-tie row (n > 5 and n S2 - S1^2 == 2 n^2) among its episodes.

Dictionaries with float keys are stored as [key, value] pairs in their order.
Output (committed): tests/golden/robustness_golden.json (inputs + expected outputs).
"""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (installs the stand-in, puts the reference on sys.path)

import matplotlib  # noqa: E402

matplotlib.use("Agg")

from envs import DexterousManipulationEnv  # noqa: E402
from evaluation.robustness_analysis import analyze_robustness_results, print_robustness_report  # noqa: E402
from evaluation.robustness_tests import RobustnessTester  # noqa: E402
from policies.random_policy import RandomPolicy  # noqa: E402

FAMILIES = ("observation_noise", "dynamics_noise", "combined_noise")
REAL = dict(cfg="medium", max_steps=20, episodes=6, obs=[0.05, 0.5], dyn=[0.3, 1.0], seed=11, space_seed=7,
            reward="dense")


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
    return x


def pairs(d):
    return [[k, jsonable(v)] for k, v in d.items()]


def record(results):
    """The inputs the analysis reads (every level's metrics, keys in order) and what it returns
    and prints."""
    analysis = analyze_robustness_results(results)
    buf = io.StringIO()
    with redirect_stdout(buf):
        print_robustness_report(analysis)
    return dict(results={"baseline": {"metrics": jsonable(results["baseline"]["metrics"])},
                         **{f: pairs({k: {"metrics": r["metrics"]} for k, r in results[f].items()}) for f in FAMILIES}},
                analysis={"baseline": jsonable(analysis["baseline"]),
                          **{f + "_degradation": pairs(analysis[f + "_degradation"]) for f in FAMILIES}},
                text=buf.getvalue())


def level(rate, length):
    return {"metrics": {"grasp_success_rate": rate, "mean_episode_length": length}}


def hand_written(base_rate):
    return {"baseline": level(base_rate, 41.5),
            "observation_noise": {0.1: level(0.25, 77.0), 0.01: level(0.7, 38.25), 0.05: level(0.0, 200.0)},
            "dynamics_noise": {0.5: level(0.1, 150.125), 0.2: level(base_rate, 41.5), 0.05: level(1.0, 12.0)},
            "combined_noise": {}}


def gen_real():
    c = REAL
    space = DexterousManipulationEnv().action_space
    space.seed(c["space_seed"])
    pol = RandomPolicy(space, seed=42)
    rt = RobustnessTester(pol, G.make_cfg(c["cfg"]), reward_type=c["reward"], max_episode_steps=c["max_steps"])
    with redirect_stdout(io.StringIO()):
        res = rt.run_robustness_sweep(c["obs"], c["dyn"], num_episodes=c["episodes"], seed=c["seed"])
    every = [res["baseline"]] + [r for f in FAMILIES for r in res[f].values()]
    for r in every:  # asserted: no variance-tie row in this fixture
        assert len(r["episodes"]) == c["episodes"]
        for e in r["episodes"]:
            counts = [sum(1 for x in row if x > 0.5) for row in e["contact_history"]]
            n, s1, s2 = len(counts), sum(counts), sum(x * x for x in counts)
            assert not (n > 5 and n * s2 - s1 * s1 == 2 * n * n), e
    out = dict(c, **record(res))
    out["steps"] = [[e["episode_steps"] for e in r["episodes"]] for r in every]
    out["success"] = [[bool(e["success"]) for e in r["episodes"]] for r in every]
    print("real sweep: success rates", [r["metrics"]["grasp_success_rate"] for r in every])
    return out


def main():
    out = dict(hand_written=[dict(base_rate=b, **record(hand_written(b))) for b in (0.0, 0.6)], real=gen_real())
    path = os.path.join(HERE, "robustness_golden.json")
    with open(path, "w") as f:
        json.dump(jsonable(out), f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
