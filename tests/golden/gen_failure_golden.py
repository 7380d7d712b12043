"""Golden fixture for the failure-mode study (evaluation/failure_analysis.py,
evaluation/failure_statistics.py, evaluation/failure_taxonomy.py).

Run ONLY in the build container, after gen_golden.py's conditions hold:

    cd /tmp && python3 -B <repository>/tests/golden/gen_failure_golden.py

Imports the reference read-only (through gen_golden's gymnasium stand-in) and records what its
functions return on three inputs:

(a) the synthetic records of tests/failure_reference.py (``synthetic_records``: all six modes,
    successes, lengths 1, 5, 6, 10, 11, both tie kinds on either side of np.var's rounding),
    classified at the history pitch and at the default bound 200;
(b) the failures a real run logs: hard curriculum, 8 held-out objects x 4 episodes, loop bound
    12, RandomPolicy(seed=42) on an action space seeded with 7, analysed at the default 200 as
    evaluation/run_failure_logging.py does.  Asserted here: no tie row among them;
(c) an empty list and a list with a single-episode mode.

Output (committed): tests/golden/failure_golden.json (inputs + expected outputs).
"""
import io
import json
import os
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (installs the stand-in, puts the reference on sys.path)

import matplotlib  # noqa: E402

matplotlib.use("Agg")

import failure_reference as R  # noqa: E402  (this repository's own generator of the synthetic records)
from envs import DexterousManipulationEnv  # noqa: E402
from evaluation.evaluator import Evaluator  # noqa: E402
from evaluation.failure_analysis import (analyze_failure_modes, print_failure_statistics,  # noqa: E402
                                         print_failure_taxonomy)
from evaluation.failure_logger import FailureLogger  # noqa: E402
from evaluation.failure_statistics import (compute_correlations, compute_failure_distribution,  # noqa: E402
                                           generate_failure_report)
from evaluation.failure_taxonomy import FailureClassifier  # noqa: E402
from evaluation.heldout_objects import HeldOutObjectSet  # noqa: E402
from policies.random_policy import RandomPolicy  # noqa: E402

SYNTHETIC = dict(E=260, max_steps=37, seed=11)
REAL = dict(heldout=["hard", 8, 42], K=4, seed=42, max_steps=12, space_seed=7, classify_max_steps=200)


def printed(fn, *args, **kw):
    buf = io.StringIO()
    with redirect_stdout(buf):
        out = fn(*args, **kw)
    return out, buf.getvalue()


def analysis_record(episodes, max_steps):
    """analyze_failure_modes / get_failure_statistics without the episode lists (each replaced by
    the indices of its episodes), and print_failure_statistics' text."""
    eps = [dict(e) for e in episodes]
    try:
        st = analyze_failure_modes(eps, max_steps=max_steps)
    except ZeroDivisionError:  # the reference divides by the episode count (failure_taxonomy.py:305)
        return "ZeroDivisionError"
    where = {id(e): i for i, e in enumerate(eps)}
    classified = {(m.value if m else "success"): [where[id(e)] for e in v]
                  for m, v in st.pop("classified_episodes").items()}
    for v in st["detailed_analysis"].values():
        v["episodes"] = [where[id(e)] for e in v["episodes"]]
    _, text = printed(print_failure_statistics, st)
    return dict(statistics=G_jsonable(st), classified=classified, text=text,
                modes=[e["failure_mode"] for e in eps], confidences=[e["failure_confidence"] for e in eps])


def logged_form(episodes, max_steps):
    """The failed episodes as FailureLogger entries (failure_logger.py:84-110), minus timestamps
    and trajectories: what failure_statistics' functions read.  Not stored: the tests rebuild
    them from the inputs and the recorded modes (tests/test_failure_stats_host.py ``entries_of``)."""
    with tempfile.TemporaryDirectory() as d:
        fl = FailureLogger(log_dir=d, save_full_trajectories=False)
        for e in episodes:
            if e["success"]:
                continue
            p = e["object_properties"]
            fl.log_episode(dict(e, object_size=p["size"], object_mass=p["mass"],
                                friction_coefficient=p["friction_coefficient"]), max_steps=max_steps)
        return [{k: v for k, v in e.items() if k not in ("timestamp", "contact_history")} for e in fl.logged_episodes]


def report_record(entries):
    with tempfile.TemporaryDirectory() as d:
        res, text = printed(generate_failure_report, [dict(e) for e in entries], output_dir=d)
        files = sorted(os.listdir(d))
        saved = json.load(open(os.path.join(d, "failure_analysis.json"))) if "failure_analysis.json" in files else None
    return dict(distribution=compute_failure_distribution(entries), correlations=compute_correlations(entries),
                report=res, report_text=text.replace(d, "<out>"), report_json=saved, files=files)


def G_jsonable(x):
    if isinstance(x, dict):
        return {str(k.value if hasattr(k, "value") else k): G_jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [G_jsonable(v) for v in x]
    if isinstance(x, (np.bool_, bool)):
        return bool(x)
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    return x


def gen_synthetic():
    d = R.synthetic_records(**SYNTHETIC)
    eps = R.episode_dicts(d)
    out = dict(SYNTHETIC, length=d["length"].tolist(), success=d["success"].tolist(),
               contacts=d["contacts"].tolist(), props=d["props"].tolist(),
               counts=[d["hist"][e, :d["length"][e]].tolist() for e in range(len(eps))], bounds={})
    for bound in (SYNTHETIC["max_steps"], 200):
        rec = analysis_record(eps, bound)
        entries = logged_form([dict(e) for e in eps], bound)
        rec.update(**report_record(entries))
        out["bounds"][str(bound)] = rec
    return out


def gen_real():
    c = REAL
    h = HeldOutObjectSet(G.make_cfg(c["heldout"][0]), num_heldout_objects=c["heldout"][1], seed=c["heldout"][2])
    space = DexterousManipulationEnv().action_space
    space.seed(c["space_seed"])
    pol = RandomPolicy(space, seed=42)
    with tempfile.TemporaryDirectory() as d:
        fl = FailureLogger(log_dir=d, save_full_trajectories=False)
        ev = Evaluator(pol, h, reward_type="dense", max_episode_steps=c["max_steps"], failure_logger=fl)
        res = ev.evaluate_heldout_set(num_episodes_per_object=c["K"], seed=c["seed"])
        logged = [dict(e) for e in fl.logged_episodes]
    # run_failure_logging.py:83-94: the logged failures (their contact lists start with the reset's
    # contacts, evaluator.py:126), classified at the default bound
    eps = [{"success": False, "episode_steps": e["episode_steps"], "num_contacts": e["num_contacts"],
            "final_contacts": e["final_contacts"], "contact_history": e["contact_history"]} for e in logged]
    all_eps = res["all_episodes"]
    # every episode of the run (successes included), as the device study sees them
    every = [{"success": e["success"], "episode_steps": e["episode_steps"], "num_contacts": e["num_contacts"],
              "final_contacts": e["final_contacts"], "contact_history": e["contact_history"],
              "object_properties": {"size": e["object_size"], "mass": e["object_mass"],
                                    "friction_coefficient": e["friction_coefficient"]}} for e in all_eps]
    for e in every:  # asserted: no tie row in this fixture
        counts = [sum(1 for x in row if x > 0.5) for row in e["contact_history"]]
        n, s1, s2 = len(counts), sum(counts), sum(x * x for x in counts)
        num = n * s2 - s1 * s1
        assert not (n > 5 and num == 2 * n * n) and not (n > 1 and num == n * n and 1 <= e["num_contacts"] <= 2), e
    bound = c["classify_max_steps"]
    rec = analysis_record(every, bound)
    logged_only = analysis_record(eps, bound)
    logged_only["episodes"] = [dict({k: v for k, v in e.items() if k != "contact_history"},
                                    counts=[sum(1 for x in row if x > 0.5) for row in e["contact_history"]])
                               for e in eps]
    entries = logged_form([dict(e) for e in every], bound)
    rec.update(logged_only=logged_only, **report_record(entries))
    per_object = {}
    for o in range(c["heldout"][1]):
        sub = every[o * c["K"]:(o + 1) * c["K"]]
        r = analysis_record(sub, bound)
        ent = logged_form([dict(e) for e in sub], bound)
        r.update(distribution=compute_failure_distribution(ent), correlations=compute_correlations(ent))
        per_object[str(o)] = r
    rec.update(per_object=per_object, steps=[e["episode_steps"] for e in all_eps],
               counts=[[sum(1 for x in row if x > 0.5) for row in e["contact_history"]] for e in all_eps])
    print("real run:", rec["statistics"]["failed_episodes"], "failures,", rec["statistics"]["failure_counts"])
    return dict(c, **rec)


def gen_edges():
    one = R.episode_dicts(R.synthetic_records(**SYNTHETIC), idx=range(12))
    clf = FailureClassifier()
    kept, seen = [], {}
    for e in one:  # two episodes of one mode and a single episode of another
        m, _ = clf.classify(e, 200)
        if m is None:
            continue
        seen[m] = seen.get(m, 0) + 1
        if (len(seen) == 1 and seen[m] <= 2) or (len(seen) == 2 and seen[m] == 1):
            kept.append(e)
    assert sorted(seen[m] for m in list(seen)[:2])[0] >= 1 and len(kept) == 3
    out = {}
    for name, eps in (("empty", []), ("single_mode_member", kept)):
        rec = analysis_record(eps, 200)
        entries = logged_form([dict(e) for e in eps], 200)
        r = dict(episodes=[{k: v for k, v in e.items() if k != "contact_history"} for e in eps],
                 counts=[[sum(1 for x in row if x > 0.5) for row in e["contact_history"]] for e in eps],
                 analysis=rec)
        r.update(report_record(entries))
        out[name] = r
    return out


def taxonomy_skeleton():
    """print_failure_taxonomy's text without the description and indicator lines (free text of the
    reference's definitions, which this repository words itself)."""
    _, text = printed(print_failure_taxonomy)
    return [ln for ln in text.split("\n") if not ln.startswith("  Description:") and not ln.startswith("    - ")]


def main():
    out = dict(synthetic=gen_synthetic(), real=gen_real(), edges=gen_edges(), taxonomy_text=taxonomy_skeleton())
    path = os.path.join(HERE, "failure_golden.json")
    with open(path, "w") as f:
        json.dump(G_jsonable(out), f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
