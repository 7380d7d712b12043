"""CPU checks of the training-run summary (dxrl_study_summarize): the NumPy restatement of both
passes (tests/study_summary_reference.py) against the reference-shaped host functions
(ablation._summarise / compute_ablation_statistics, curriculum_ablation.compute_convergence_metrics
/ aggregate_metrics), the host half of summarize_runs (tie settle, dictionaries from the tables),
and the C ABI of the new entry point."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from dexterous_rl_manipulation_amd import ablation as A
from dexterous_rl_manipulation_amd import curriculum_ablation as CA

import study_summary_cases as K
import study_summary_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dxrl.h")
W, THR = K.W, K.THR
CFG = A.AblationConfig(True, True, "x")


def tables(case):
    return S.lane_pass(case["ep_return"], case["ep_length"], case["ep_success"], case["ep_level"], case["episodes"],
                       W, CA.min_successes(W, 0.5), THR)


def reference_metrics(case, l):
    r, _, ok = K.lane_records(case, l)
    return CA.compute_convergence_metrics(list(r), [1.0 if s else 0.0 for s in ok], W, THR)


def test_min_successes():
    assert CA.min_successes(20, 0.5) == 10 == K.C_MIN


@pytest.mark.parametrize("case", [K.random_ragged, K.random_uniform, K.crafted])
def test_lane_columns_equal_summarise(case):
    c = case()
    ints, reals, status = tables(c)
    assert status == 0
    assert sorted(set(c["episodes"].tolist()) & set(K.E_SIZES)) == K.E_SIZES or case is not K.random_ragged
    for l in range(len(ints)):
        r, steps, ok = K.lane_records(c, l)
        want = A._summarise(CFG, r, steps, ok, len(r))
        E = len(r)
        assert ints[l, S.EPISODES] == E and c["cap"] >= E
        assert ints[l, S.FINAL_WINDOW] / min(W, E) == want.final_success_rate
        assert ints[l, S.STEPS] / E == want.mean_episode_length
        assert (None if ints[l, S.CONV] < 0 else int(ints[l, S.CONV])) == want.convergence_step
        assert ints[l, S.LEVEL] == (-1 if c["ep_level"] is None else c["ep_level"][l, E - 1])


@pytest.mark.parametrize("case", [K.random_ragged, K.random_uniform, K.crafted])
def test_lane_rows_equal_compute_convergence_metrics(case):
    c = case()
    ints, reals, _ = tables(c)
    ties = [l for l in range(len(ints)) if ints[l, S.FLAGS] & S.FLAG_TIE]
    assert ties == ([K.CRAFTED.index("all_thr")] if case is K.crafted else [])  # the random inputs have none
    for l in range(len(ints)):
        if l in ties:
            continue
        want = reference_metrics(c, l)
        got = CA.lane_metrics_row(ints[l], reals[l], W)
        assert list(got) == list(want)
        for k in ("convergence_episode", "final_success_rate", "overall_success_rate"):
            assert got[k] == want[k], (l, k)
        scale = np.abs(K.lane_records(c, l)[0]).max()
        for k in ("reward_variance", "reward_std", "final_reward", "mean_reward", "convergence_steps"):
            if want[k] is None:
                assert got[k] is None, (l, k)
            else:
                s = scale * scale if k == "reward_variance" else scale * max(1, want["convergence_episode"] or 1) \
                    if k == "convergence_steps" else scale
                assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]) + 1e-12 * s, (l, k)
        if np.isinf(want["coefficient_of_variation"]):
            assert np.isinf(got["coefficient_of_variation"])
        else:
            # std / mean with both within the bound above: the errors of std and of mean over |mean|
            cv, mean = want["coefficient_of_variation"], abs(want["mean_reward"])
            tol = 1e-12 * abs(cv) + 2e-12 * (abs(want["reward_std"]) + scale) * (1 + abs(cv)) / mean
            assert abs(got["coefficient_of_variation"] - cv) <= tol, l


def test_crafted_lanes():
    c = K.crafted()
    ints, reals, _ = tables(c)
    row = {n: ints[i] for i, n in enumerate(K.CRAFTED)}
    assert row["conv_at_w"][S.CONV] == W
    assert row["conv_at_last"][S.CONV] == 39 == row["conv_at_last"][S.EPISODES] - 1
    assert row["nine_of_20"][S.CONV] == -1 and row["ten_of_20"][S.CONV] == 20
    assert row["straddle_64"][S.CONV] == 65
    assert row["E_eq_w"][S.CONV] == -1 and row["E_eq_w"][S.FINAL_WINDOW] == 20
    assert row["E_lt_w"][S.CONV] == -1 and row["E_lt_w"][S.FINAL_WINDOW] == 3 and row["E_lt_w"][S.REWARD_CONV] == W - 1
    assert row["cross_late"][S.REWARD_CONV] == 38 and not row["cross_late"][S.FLAGS]
    z = CA.lane_metrics_row(row["zero_mean"], reals[K.CRAFTED.index("zero_mean")], W)
    assert z["mean_reward"] == 0.0 and z["coefficient_of_variation"] == np.inf and z["convergence_episode"] is None
    assert row["all_thr"][S.FLAGS] == S.FLAG_TIE
    # twenty products of 0.5 * (1 / 20) summed left to right and np.convolve's sum need not agree
    assert abs(S.moving_average(np.full(20, THR), 20)[0][0] - THR) <= 64 * np.finfo(float).eps


def groups_of(case):
    if case is K.random_uniform:
        return {"a": [0, 1, 2, 3], "b": [4, 5, 6, 7], "c": [8, 9, 10, 11], "seed0": [0, 4, 8], "all": list(range(12)),
                "twice": [5, 5, 6]}
    if case is K.crafted:
        i = K.CRAFTED.index
        return {"forty": [i(n) for n in ("conv_at_w", "conv_at_last", "nine_of_20", "ten_of_20", "all_thr")],
                "none_converged": [i("nine_of_20"), i("zero_mean"), i("all_thr")], "mixed": list(range(len(K.CRAFTED))),
                "inf_cv": [i("zero_mean"), i("ten_of_20")]}
    return {"all": list(range(16)), "long": [8, 9], "one": [0]}


def csr(groups):
    m = [np.asarray(v, dtype=np.int32) for v in groups.values()]
    off = np.zeros(len(m) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in m])
    return off, np.concatenate(m), m


def close(got, want, path=""):
    if isinstance(want, dict):
        assert set(got) == set(want), path
        for k in want:
            close(got[k], want[k], f"{path}.{k}")
    elif want is None or isinstance(want, int):
        assert got == want, path
    elif np.isnan(want) or np.isinf(want):
        assert (np.isnan(got) and np.isnan(want)) or got == want, path
    else:
        assert got == pytest.approx(want, rel=1e-12, abs=1e-15), path


@pytest.mark.parametrize("case", [K.random_ragged, K.random_uniform, K.crafted])
def test_group_tables_give_reference_statistics(case):
    c = case()
    ints, reals, _ = tables(c)
    groups = groups_of(case)
    off, flat, members = csr(groups)
    stats, metrics, ties, tie_count, status = S.group_pass(ints, reals, off, flat, tie_cap=len(ints))
    mixed = any(len({int(ints[l, S.EPISODES]) for l in m}) > 1 for m in members)
    assert status == (S.ST_MIXED if mixed else 0) and tie_count == len(ties)
    if case is K.crafted:
        g = list(groups).index("none_converged")
        assert stats[g, 8] == 0 and stats[g, 14] == 1 and stats[list(groups).index("forty"), 14] == 1
        assert metrics[list(groups).index("inf_cv"), 2, 0] == 1  # the infinite CV is left out
    out = CA.form_summary(ints, reals, stats, metrics, ties, list(groups), members, W, THR,
                          lambda row: K.lane_records(c, row)[0], return_runs=True)
    for name, m in groups.items():
        runs = []
        for l in m:
            r, steps, ok = K.lane_records(c, l)
            runs.append(A._summarise(CFG, r, steps, ok, len(r)))
        close(out["statistics"][name], A.compute_ablation_statistics({name: runs})[name], name)
        with np.errstate(invalid="ignore"):
            want = CA.aggregate_metrics([reference_metrics(c, l) for l in m])
        close(out["aggregated_metrics"][name], want, name)
    if case is K.crafted:
        assert out["statistics"]["none_converged"]["convergence_step"] == {"mean": None, "std": None,
                                                                           "num_converged": 0}
        t = K.CRAFTED.index("all_thr")  # settled: the lane now says what the reference function says
        assert out["tie_lanes"] == [t]
        assert out["runs"][t]["convergence_episode"] == reference_metrics(c, t)["convergence_episode"]
        assert np.isinf(out["aggregated_metrics"]["inf_cv"]["coefficient_of_variation"]["mean"])


def test_status_bits_of_the_restatement():
    c = K.random_uniform()
    eps = c["episodes"].copy()
    eps[3], eps[5] = 0, c["cap"] + 1
    ints, reals, status = S.lane_pass(c["ep_return"], c["ep_length"], c["ep_success"], None, eps, W, 10, THR)
    assert status == S.ST_LANE and ints[3, S.FLAGS] == S.FLAG_SKIPPED == ints[5, S.FLAGS]
    stats, _, _, _, st = S.group_pass(ints, reals, [0, 4, 6], [0, 1, 2, 3, 4, 5], 12)
    assert st == 0 and stats[0, 0] == 3 and stats[1, 0] == 1  # skipped lanes are left out
    assert S.group_pass(ints, reals, [0, 7], [0, 1, 2, 3, 4, 5], 12)[4] & S.ST_RANGE
    assert S.group_pass(ints, reals, [0, 2], [0, 12], 12)[4] & S.ST_RANGE
    ic, rc, _ = tables(K.crafted())
    assert S.group_pass(ic, rc, [0, 1], [0], 0)[3:] == (1, S.ST_TIE_CAP)


def test_two_buffers_with_offset_equal_one():
    c = K.random_ragged()
    whole = tables(c)
    ints = np.zeros((16, S.LANE_INTS), dtype=np.int64)
    reals = np.zeros((16, S.LANE_REALS))
    for lo, hi in ((0, 6), (6, 16)):
        S.lane_pass(c["ep_return"][lo:hi], c["ep_length"][lo:hi], c["ep_success"][lo:hi], c["ep_level"][lo:hi],
                    c["episodes"][lo:hi], W, 10, THR, ints, reals, lane_offset=lo)
    assert np.array_equal(ints, whole[0]) and np.array_equal(reals, whole[1])


@pytest.fixture(scope="module")
def native():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        d.build.build_native()
    return _native


def test_study_summary_struct_layout_matches_c(native):
    """dxrl_study_summary_args against its ctypes mirror, by a gcc-compiled probe."""
    s, mirror = "dxrl_study_summary_args", native.StudySummaryArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));', 'printf("abi %d\\n", DXRL_ABI_VERSION);',
             'printf("ints %d\\n", DXRL_STUDY_LANE_INTS);', 'printf("reals %d\\n", DXRL_STUDY_LANE_REALS);',
             'printf("metrics %d\\n", DXRL_STUDY_METRICS);']
    for f, _ in mirror._fields_:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        open(src, "w").write("\n".join(lines))
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got[s]) == C.sizeof(mirror)
    for f, _ in mirror._fields_:
        assert int(got[f"{s}.{f}"]) == getattr(mirror, f).offset, f
    assert int(got["abi"]) == native.ABI_VERSION == 1
    assert (int(got["ints"]), int(got["reals"]), int(got["metrics"])) == \
        (native.STUDY_LANE_INTS, native.STUDY_LANE_REALS, native.STUDY_METRICS) == (S.LANE_INTS, S.LANE_REALS, S.METRICS)


def test_entry_rejects_bad_arguments_before_any_launch(native):
    a = native.StudySummaryArgs()
    fake = 1 << 20  # never dereferenced: the checks run first
    with pytest.raises(ValueError, match="null args"):
        native.call("dxrl_study_summarize", 0, None, None)

    def fill():
        a.num_lanes, a.record_cap, a.lane_offset, a.total_lanes, a.window, a.min_count = 4, 10, 0, 4, 20, 10
        for k in ("ep_return", "ep_length", "ep_success", "lane_episodes", "lane_ints", "lane_reals", "status"):
            setattr(a, k, fake)

    for field, value, msg in (("window", 0, "window"), ("window", 65, "window"), ("record_cap", 0, "record_cap"),
                              ("lane_offset", 1, "lane table"), ("lane_offset", -1, "lane table"),
                              ("ep_return", None, "null episode record"), ("lane_episodes", None, "lane_episodes"),
                              ("lane_ints", None, "null lane_ints"), ("status", None, "status")):
        fill()
        setattr(a, field, value)
        with pytest.raises(ValueError, match=msg):
            native.call("dxrl_study_summarize", 0, C.byref(a), None)
    fill()
    a.group_stats = fake
    with pytest.raises(ValueError, match="group_metrics"):
        native.call("dxrl_study_summarize", 0, C.byref(a), None)
