"""CPU tests of the failure-mode study (failure_analysis.py, failure_statistics.py) against what
the reference's functions returned (tests/golden/failure_golden.json, written by
tests/golden/gen_failure_golden.py):

1. ``analyze_failure_modes`` / ``get_failure_statistics`` / ``compute_failure_distribution`` /
   ``compute_correlations`` dictionaries, ``print_failure_statistics`` and
   ``generate_failure_report`` text, the report's JSON and both PNGs, on (a) the synthetic records,
   (b) the real run's episodes and (c) the edge inputs.  ``print_failure_taxonomy`` is compared
   without its description / indicator lines: those are free text of the reference's definitions,
   which failures.FAILURE_MODE_DEFINITIONS words itself.
2. the restatement of both kernels (tests/failure_reference.py) against the golden
   classifications: modes exact outside tie rows, exact after the host settle, confidences within
   1e-12 relative (the integer restatement rounds the variance once, np.var several times;
   6.6e-16 was measured on 60,000 random histories); and the dictionaries built from its tables
   (``tables_to_dicts``) against the golden ones at the 1e-9 bar of the group moments.
3. ``dxrl_failure_summary_args`` and ``dxrl_eval_args`` against their ctypes mirrors.
"""
import contextlib
import ctypes as C
import io
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import failure_reference as R
from dexterous_rl_manipulation_amd import failure_analysis as fa
from dexterous_rl_manipulation_amd import failure_statistics as fs
from dexterous_rl_manipulation_amd.failures import FailureClassifier

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "failure_golden.json")
HEADER = os.path.join(os.path.dirname(HERE), "include", "dxrl.h")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def hist_of(counts):
    return [[1.0 if j < c else 0.0 for j in range(5)] for c in counts]


def synthetic_episodes(g):
    s = g["synthetic"]
    return [{"success": bool(s["success"][e]), "episode_steps": s["length"][e], "num_contacts": s["contacts"][e],
             "final_contacts": s["contacts"][e], "contact_history": hist_of(s["counts"][e]),
             "object_properties": dict(zip(("size", "mass", "friction_coefficient"), s["props"][e]))}
            for e in range(s["E"])]


def real_episodes(g):
    """Fixture (b) rebuilt from the golden inputs: the run's episodes, object-major."""
    from dexterous_rl_manipulation_amd import evaluation as ev
    from test_eval_host import cfg_of
    r = g["real"]
    objs = ev.HeldOutObjectSet(cfg_of(r["heldout"][0]), num_heldout_objects=r["heldout"][1],
                               seed=r["heldout"][2]).heldout_objects
    out = []
    for i, (n, counts) in enumerate(zip(r["steps"], r["counts"])):
        o = objs[i // r["K"]]
        out.append({"success": r["modes"][i] is None, "episode_steps": n, "num_contacts": counts[-1],
                    "final_contacts": counts[-1], "contact_history": hist_of(counts),
                    "object_properties": {"size": o.size, "mass": o.mass, "friction_coefficient": o.friction}})
    return out


def entries_of(episodes):
    """The failed episodes (classified in place by analyze_failure_modes) in the logged form."""
    return [{k: v for k, v in e.items() if k != "contact_history"} for e in episodes if e.get("failure_mode")]


def printed(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*args, **kw)
    return out, buf.getvalue()


def check_analysis(episodes, want, bound):
    eps = [dict(e) for e in episodes]
    st = fa.analyze_failure_modes(eps, max_steps=bound)
    where = {id(e): i for i, e in enumerate(eps)}
    classified = {(m.value if m else "success"): [where[id(e)] for e in v]
                  for m, v in st.pop("classified_episodes").items()}
    assert classified == want["classified"]
    for v in st["detailed_analysis"].values():
        v["episodes"] = [where[id(e)] for e in v["episodes"]]
    assert st == want["statistics"]
    assert list(st["detailed_analysis"]) == list(want["statistics"]["detailed_analysis"])
    assert printed(fa.print_failure_statistics, st)[1] == want["text"]
    assert [e["failure_mode"] for e in eps] == want["modes"]
    assert [e["failure_confidence"] for e in eps] == want["confidences"]
    plain = FailureClassifier().get_failure_statistics([dict(e) for e in episodes], bound)
    plain.pop("classified_episodes")
    assert plain == {k: v for k, v in want["statistics"].items() if k != "detailed_analysis"}
    return eps


def check_report(entries, want, tmp_path):
    assert fs.compute_failure_distribution(entries) == want["distribution"]
    assert list(fs.compute_failure_distribution(entries)) == list(want["distribution"])
    assert fs.compute_correlations(entries) == want["correlations"]
    res, text = printed(fs.generate_failure_report, [dict(e) for e in entries], output_dir=str(tmp_path))
    assert res == want["report"]
    assert text.replace(str(tmp_path), "<out>") == want["report_text"]
    assert sorted(os.listdir(tmp_path)) == want["files"]
    if want["report_json"] is not None:
        with open(tmp_path / "failure_analysis.json") as f:
            assert json.load(f) == want["report_json"]
        for png in ("failure_distribution.png", "failure_correlations.png"):
            assert (tmp_path / png).stat().st_size > 0


# ------------------------------------------------------------------ 1. host functions
@pytest.mark.parametrize("bound", [37, 200])
def test_synthetic_records_match_reference(golden, bound, tmp_path):
    want = golden["synthetic"]["bounds"][str(bound)]
    eps = check_analysis(synthetic_episodes(golden), want, bound)
    assert set(m for m in want["modes"] if m) == set(R.MODE_NAMES) - ({"timeout"} if bound == 200 else set())
    check_report(entries_of(eps), want, tmp_path)


def test_real_run_matches_reference(golden, tmp_path):
    r = golden["real"]
    eps = check_analysis(real_episodes(golden), r, r["classify_max_steps"])
    assert r["statistics"]["failed_episodes"] == 17 and len(r["statistics"]["detailed_analysis"]) == 2
    check_report(entries_of(eps), r, tmp_path)
    K = r["K"]
    for o in range(r["heldout"][1]):
        sub = check_analysis(real_episodes(golden)[o * K:(o + 1) * K], r["per_object"][str(o)],
                             r["classify_max_steps"])
        assert fs.compute_failure_distribution(entries_of(sub)) == r["per_object"][str(o)]["distribution"]
        assert fs.compute_correlations(entries_of(sub)) == r["per_object"][str(o)]["correlations"]
    # run_failure_logging.py's own call: the logged failures (contact lists that start with the
    # reset's contacts), at the default bound
    lo = r["logged_only"]
    check_analysis([dict({k: v for k, v in e.items() if k != "counts"}, contact_history=hist_of(e["counts"]))
                    for e in lo["episodes"]], lo, r["classify_max_steps"])


def test_edge_inputs_match_reference(golden, tmp_path):
    e = golden["edges"]["empty"]
    assert e["analysis"] == "ZeroDivisionError"
    with pytest.raises(ZeroDivisionError):
        fa.analyze_failure_modes([])
    check_report([], e, tmp_path / "empty")
    s = golden["edges"]["single_mode_member"]
    eps = check_analysis([dict(ep, contact_history=hist_of(c)) for ep, c in zip(s["episodes"], s["counts"])],
                         s["analysis"], 200)
    entries = entries_of(eps)
    assert len(s["distribution"]) == 2 and len(s["correlations"]) == 1  # the single-episode mode is skipped
    check_report(entries, s, tmp_path / "single")


def test_taxonomy_text_and_log_round_trip(golden, tmp_path):
    _, text = printed(fa.print_failure_taxonomy)
    skeleton = [ln for ln in text.split("\n") if not ln.startswith("  Description:") and not ln.startswith("    - ")]
    assert skeleton == golden["taxonomy_text"]
    path = tmp_path / "log.json"
    path.write_text(json.dumps({"metadata": {}, "episodes": [{"episode_id": 0}]}))
    assert fs.load_failure_logs(str(path)) == [{"episode_id": 0}]
    path.write_text("{}")
    assert fs.load_failure_logs(str(path)) == []
    _, out = printed(fs.main, ["--log_file", str(tmp_path / "missing.json"), "--output_dir", str(tmp_path)])
    assert "File not found" in out


def test_exports():
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import evaluation as ev
    for name in ("print_failure_taxonomy", "print_failure_statistics", "analyze_failure_modes", "load_failure_logs",
                 "compute_failure_distribution", "compute_correlations", "plot_failure_distribution",
                 "plot_failure_correlations", "generate_failure_report", "run_failure_study"):
        assert callable(getattr(ev, name)), name
    assert pkg.failure_statistics is fs and pkg.failure_analysis is fa


# ------------------------------------------------------------------ 2. the kernels' restatement
def synthetic_arrays(golden):
    s = golden["synthetic"]
    d = R.synthetic_records(s["E"], s["max_steps"], s["seed"])
    assert d["length"].tolist() == s["length"] and d["contacts"].tolist() == s["contacts"]
    assert [d["hist"][e, :d["length"][e]].tolist() for e in range(s["E"])] == s["counts"]
    assert d["props"].tolist() == s["props"]
    return d


def golden_codes(want):
    mode = np.array([-1 if m is None else R.MODE_NAMES.index(m) for m in want["modes"]])
    conf = np.array([next(iter(c.values())) if c else 0.0 for c in want["confidences"]])
    return mode, conf


@pytest.mark.parametrize("bound", [37, 200])
def test_restatement_matches_golden_classifications(golden, bound):
    d = synthetic_arrays(golden)
    ms = golden["synthetic"]["max_steps"]
    want_mode, want_conf = golden_codes(golden["synthetic"]["bounds"][str(bound)])
    mom = R.moments_of(d["hist"], d["length"], ms)
    mode, conf, tie = R.episode_pass(d["length"], d["success"], d["contacts"], mom, ms, bound)
    assert np.array_equal(mode[~tie], want_mode[~tie])
    n = d["length"].astype(np.int64)
    num = n * mom[:, 1] - mom[:, 0].astype(np.int64) ** 2
    assert (tie & (num == 2 * n * n)).sum() >= 2 and (tie & (num == n * n)).sum() >= 2  # both tie kinds
    final, fconf = R.settle(mode, conf, tie, d["length"], d["contacts"], d["hist"])
    moved = final != mode
    assert np.array_equal(final, want_mode)
    assert (moved & (num == 2 * n * n)).any() and (moved & (num == n * n)).any()  # np.var moved one of each
    assert (tie & ~moved & (num == 2 * n * n)).any() and (tie & ~moved & (num == n * n)).any()
    rel = np.abs(fconf - want_conf) / np.maximum(np.abs(want_conf), 1e-300)
    print("worst relative confidence error", rel.max())
    assert rel.max() <= 1e-12
    assert set(np.unique(want_conf[want_mode == R.SLIPPAGE])) - {1.0} and (want_conf[want_mode == R.UNSTABLE] < 1).any()


def close(got, want, scale):
    return abs(got - want) <= 1e-9 * scale


@pytest.mark.parametrize("bound", [37, 200])
def test_tables_to_dicts_match_golden(golden, bound):
    """Restatement tables (history form: tie rows left out, then settled and merged on the host as
    the device path does) -> dictionaries == the reference's on the same records."""
    from dexterous_rl_manipulation_amd import evaluator as evr
    d = synthetic_arrays(golden)
    ms, E = golden["synthetic"]["max_steps"], golden["synthetic"]["E"]
    want = golden["synthetic"]["bounds"][str(bound)]
    mom = R.moments_of(d["hist"], d["length"], ms)
    mode, conf, tie = R.episode_pass(d["length"], d["success"], d["contacts"], mom, ms, bound)
    groups = [np.arange(E)]
    stats, totals, mp = R.group_pass(mode, tie, tie, d["length"], d["success"], d["contacts"], d["props"], groups)
    off, mem = evr.group_table(groups)
    rows = np.flatnonzero(tie)
    evr.settle_failure_ties(stats, mp, off, mem, rows, d["hist"][rows], d["length"][rows], d["contacts"][rows],
                            d["props"][rows], bound, 3)
    got = fs.tables_to_dicts(stats, totals, mp, 0)
    st = {k: v for k, v in want["statistics"].items()}
    detailed = {k: {kk: vv for kk, vv in v.items() if kk != "episodes"} for k, v in st.pop("detailed_analysis").items()}
    assert got["statistics"].pop("detailed_analysis") == detailed
    assert got["statistics"] == st
    check_dicts(got, want)


def check_dicts(got, want):
    """``distribution`` / ``correlations`` of a study against the reference's: counts, frequencies,
    min and max exact, means and standard deviations within 1e-9 max(|mean|, std)."""
    assert set(got["distribution"]) == set(want["distribution"])
    assert set(got["correlations"]) == set(want["correlations"])
    for m, w in want["distribution"].items():
        g = got["distribution"][m]
        assert g["count"] == w["count"] and g["frequency"] == w["frequency"]
        assert g["mean_final_contacts"] == w["mean_final_contacts"] and g["mean_episode_length"] == w["mean_episode_length"]
        for mean_key, std_key in (("mean_episode_length", "std_episode_length"),
                                  ("mean_object_size", "std_object_size"), ("mean_object_mass", "std_object_mass"),
                                  ("mean_friction", "std_friction")):
            scale = max(abs(w[mean_key]), w[std_key])
            assert close(g[mean_key], w[mean_key], scale) and close(g[std_key], w[std_key], scale), (m, mean_key)
    for m, w in want["correlations"].items():
        g = got["correlations"][m]
        for key, sub in w.items():
            scale = max(abs(sub["mean"]), sub["std"])
            assert close(g[key]["mean"], sub["mean"], scale) and close(g[key]["std"], sub["std"], scale), (m, key)
            if "min" in sub:
                assert g[key]["min"] == sub["min"] and g[key]["max"] == sub["max"]


# ------------------------------------------------------------------ 3. struct layouts
@pytest.mark.parametrize("struct,mirror", [("dxrl_failure_summary_args", "FailureSummaryArgs"),
                                           ("dxrl_eval_args", "EvalArgs")])
def test_struct_layout_matches_c(struct, mirror):
    """sizeof and every field offset against the ctypes mirror, by a gcc-compiled probe."""
    from dexterous_rl_manipulation_amd import _native as N
    mirror = getattr(N, mirror)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{struct} %zu\\n", sizeof({struct}));', 'printf("modes %d\\n", DXRL_FAILURE_MODES);']
    for f, _ in mirror._fields_:
        lines.append(f'printf("{struct}.{f} %zu\\n", offsetof({struct}, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        with open(c, "w") as f:
            f.write("\n".join(lines))
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got[struct]) == C.sizeof(mirror)
    for f, _ in mirror._fields_:
        assert int(got[f"{struct}.{f}"]) == getattr(mirror, f).offset, f
    assert int(got["modes"]) == N.FAILURE_MODES == len(R.MODE_NAMES)
    assert mirror._fields_[-1][0] == {"EvalArgs": "hist_moments", "FailureSummaryArgs": "status"}[mirror.__name__]
