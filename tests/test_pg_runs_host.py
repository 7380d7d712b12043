"""CPU checks of the run-set summary (dxrl_pg_runs_summarize) and of the study layer above it: the
NumPy restatement (tests/pg_runs_reference.py) against np.mean / np.std,
reward_comparison.window_convergence and ablation.compute_ablation_statistics on crafted runs
(tests/pg_runs_cases.py); the package's own host path against the restatement; the C ABI of the new
entry point (argument checks before any launch, struct layout against a gcc-compiled header); and
the report, the JSON and the command's arguments on a synthetic StudyResult."""
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from dexterous_rl_manipulation_amd import ablation as A
from dexterous_rl_manipulation_amd import curriculum_ablation as CA
from dexterous_rl_manipulation_amd import reward_comparison as RC

import pg_runs_cases as K
import pg_runs_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dxrl.h")
EPS = 2.0 ** -52


@pytest.fixture(scope="module", params=[24, 16], ids=["log_cols", "val_cols"])
def case(request):
    t = K.slab(request.param)
    off, flat = K.csr()
    return {"tables": t, "off": off, "flat": flat, "out": P.summarize(t, K.RUN_ROWS, K.SPECS, off, flat, K.CONTRASTS)}


def column(case, r, col):
    return case["tables"][r, :K.RUN_ROWS[r], col]


# ------------------------------------------------------------------ the run pass
def test_run_rows_against_numpy_and_window_convergence(case):
    run_table = case["out"][0]
    for r in range(K.R):
        for s, (col, x_col, w, thr, fw) in enumerate(K.SPECS):
            v, row = column(case, r, col), run_table[r, s]
            n = len(v)
            assert row[P.ROWS] == n and row[P.NAN_ROWS] == np.isnan(v).sum()
            ok = v[~np.isnan(v)]
            if n == 0:
                assert np.isnan(row[[P.FINAL, P.BEST, P.X_AT_CONV, P.CURVE_MEAN]]).all()
                assert row[P.BEST_ROW] == -1 and row[P.CONV] == -1
                continue
            tail = v[-min(fw, n):]
            if np.isnan(tail).any():
                assert np.isnan(row[P.FINAL])
            else:
                assert abs(row[P.FINAL] - np.mean(tail)) <= len(tail) * EPS * np.abs(tail).sum() / len(tail)
            if ok.size:
                assert row[P.BEST] == np.nanmax(v) and row[P.BEST_ROW] == np.flatnonzero(v == np.nanmax(v))[0]
                assert abs(row[P.CURVE_MEAN] - ok.mean()) <= ok.size * EPS * np.abs(ok).sum() / ok.size
            first = RC.window_convergence(v, w, thr)
            if first is None:
                assert row[P.CONV] == -1 and np.isnan(row[P.X_AT_CONV])
            else:
                assert row[P.CONV] == first + w - 1
                assert row[P.X_AT_CONV] == case["tables"][r, first + w - 1, x_col]
    assert not np.isin(K.SENTINEL, run_table)


def test_crafted_runs(case):
    run_table = case["out"][0]
    c = run_table[K.CRAFTED, 0]
    # the window on the threshold (rows 20 .. 23) does not converge; rows 40 .. 43 do
    assert c[P.CONV] == 43 and c[P.X_AT_CONV] == 44000.0
    assert c[P.BEST] == 0.625 and c[P.BEST_ROW] == 43      # row 60 holds the same maximum
    assert c[P.NAN_ROWS] == 1 and c[P.FINAL] == (9 * 0.25 + 0.625) / 10   # the NaN row lies before the window
    assert np.isnan(run_table[K.CRAFTED, 1, P.FINAL])      # a NaN inside the final window
    assert run_table[K.NEVER, 0, P.CONV] == -1 and run_table[K.NEVER, 0, P.BEST] == 0.5
    assert run_table[K.SHORT, 0, P.CONV] == -1 and run_table[K.SHORT, 0, P.FINAL] == 1.0
    assert run_table[K.EXACT_W, 0, P.CONV] == K.W - 1
    assert run_table[K.ONE, 0].tolist()[:5] == [1.0, 0.875, 0.875, 0.0, -1.0]
    assert run_table[K.ONE, 2, P.CONV] in (0.0, -1.0)      # W = 1 on a single row


# ------------------------------------------------------------------ the group and contrast passes
def close(got, want, rel=1e-9):
    if want is None or (isinstance(want, float) and math.isnan(want)):
        return got is None or math.isnan(got)
    return abs(got - want) <= rel * abs(want) + 1e-300


def test_group_rows_against_numpy(case):
    run_table, group_table = case["out"][:2]
    assert case["out"][3] == P.ST_CONTRAST  # only the unequal contrast is reported
    for g, mem in enumerate(K.GROUPS.values()):
        for s in range(len(K.SPECS)):
            conv = sum(run_table[r, s, P.CONV] >= 0 for r in mem)
            for k in range(P.METRICS):
                x = np.array([P.metrics_of(run_table[r, s])[k] for r in mem], dtype=np.float64)
                x = x[np.isfinite(x)]
                row = group_table[g, s, k]
                assert row[0] == x.size and row[5] == conv
                if x.size == 0:
                    assert np.isnan(row[1:5]).all()
                    continue
                assert abs(row[1] - x.mean()) <= x.size * EPS * np.abs(x).sum() / x.size
                assert abs(row[2] - x.std()) <= 1e-9 * x.std() + 4 * EPS * np.abs(x).max()
                assert row[3] == x.min() and row[4] == x.max()
    g = K.NAMES.index("none_converged")
    assert group_table[g, 0, P.M_CONV, 0] == 0 and group_table[g, 0, P.M_FINAL, 0] == 2
    assert (group_table[K.NAMES.index("empty"), :, :, 0] == 0).all()


def test_contrast_rows_against_numpy(case):
    run_table, _, contrast_table, _ = case["out"]
    groups = list(K.GROUPS.values())
    assert np.isnan(contrast_table[K.Q_UNEQUAL]).all()
    assert (contrast_table[K.Q_NOTHING, :, :, 0] == 0).all() and np.isnan(contrast_table[K.Q_NOTHING, :, :, 1:]).all()
    for q in range(K.Q_UNEQUAL):
        used = [g for g in range(len(groups)) if K.CONTRASTS[q, g] != 0.0]
        m = len(groups[used[0]])
        for s in range(len(K.SPECS)):
            for k in range(P.METRICS):
                x = np.array([[P.metrics_of(run_table[groups[g][j], s])[k] for g in used] for j in range(m)])
                d = (x * K.CONTRASTS[q, used]).sum(axis=1)
                d = d[np.isfinite(x).all(axis=1)]
                row = contrast_table[q, s, k]
                assert row[0] == d.size
                if d.size == 0:
                    assert np.isnan(row[1:]).all()
                    continue
                scale = np.abs(x).max() if np.isfinite(x).any() else 0.0
                assert abs(row[1] - d.mean()) <= 8 * EPS * (np.abs(d).sum() + np.nanmax(np.abs(x)))
                if d.size < 2:
                    assert np.isnan(row[2:]).all()
                    continue
                sd = d.std(ddof=1)
                assert abs(row[2] - sd) <= 1e-9 * sd + 8 * EPS * scale
                assert abs(row[3] - sd / math.sqrt(d.size)) <= 1e-9 * sd + 8 * EPS * scale
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = np.float64(row[1]) / np.float64(row[3])
                assert row[4] == t or (np.isnan(row[4]) and np.isnan(t))
    # the empty run has no final window: its pair is left out
    assert contrast_table[K.Q_NAN_MEMBER, 0, P.M_FINAL, 0] == 1
    # a pairwise difference and the interaction are just weight rows
    a, b, c, d = (groups[K.NAMES.index(n)] for n in ("a", "b", "none_converged", "d"))
    f = lambda r: run_table[r, 0, P.FINAL]  # noqa: E731
    want = np.mean([f(a[j]) - f(b[j]) - f(c[j]) + f(d[j]) for j in range(2)])
    assert contrast_table[2, 0, P.M_FINAL, 1] == pytest.approx(want, rel=1e-12)


def test_status_bits_of_the_restatement(case):
    t = case["tables"]
    rows = K.RUN_ROWS.copy()
    rows[K.ONE], rows[K.SHORT] = -1, K.CAP + 1
    run_table, status = P.run_pass(t, rows, K.SPECS)
    assert status == P.ST_ROWS and (run_table[[K.ONE, K.SHORT], :, P.ROWS] == 0).all()
    whole = case["out"][0]
    off, flat = K.csr({"bad": [K.CRAFTED, K.R, -1, K.NEVER], "good": [K.CRAFTED, K.NEVER]})
    gt, st = P.group_pass(whole, off, flat)
    assert st == P.ST_RANGE
    # the out-of-range members are skipped, the places of the others stay: the same statistics
    assert np.array_equal(gt[0], gt[1], equal_nan=True)
    assert P.group_pass(whole, [0, 3], [0, 1])[1] == P.ST_RANGE      # an offset past the members
    assert P.group_pass(whole, [2, 1], [0, 1, 2])[1] == P.ST_RANGE   # offsets that decrease
    ct, st = P.contrast_pass(whole, off, flat, [[1.0, 0.0]])
    assert st == 0 and ct[0, 0, P.M_FINAL, 0] == 2  # the pairs of the two in-range members


def test_statistics_dictionary_equals_compute_ablation_statistics(case):
    """pg_statistics over group tables against the reference function over per-run results."""
    from dexterous_rl_manipulation_amd import training_study as T
    result, run_table = synthetic_result(case["tables"])
    stats = A.pg_statistics(result)
    slab = result.validation
    runs = {}
    cfg = A.AblationConfig(True, True, "x")
    for a, arm in enumerate(result.arms):
        for k in range(len(result.seeds)):
            r = a * len(result.seeds) + k
            conv = run_table[r, 0, P.X_AT_CONV]
            runs.setdefault(arm, []).append(A.TrainingResults(
                cfg, [], [], [], final_success_rate=run_table[r, 0, P.FINAL],
                mean_episode_length=run_table[r, 1, P.CURVE_MEAN],
                convergence_step=None if np.isnan(conv) else conv, total_episodes=0))
    want = A.compute_ablation_statistics(runs)
    assert set(stats) == set(want) | {"effects"}
    for arm in result.arms:
        for key, entry in want[arm].items():
            for name, value in entry.items():
                got = stats[arm][key][name]
                if name == "num_converged":
                    assert got == value
                else:
                    assert close(got, value), (arm, key, name, got, value)
    assert set(stats["effects"]) == set(A.PG_COMPONENT_CONTRASTS)
    e = stats["effects"]["no_curriculum_vs_baseline"]
    n = len(result.seeds)
    d = [run_table[n + k, 0, P.FINAL] - run_table[k, 0, P.FINAL] for k in range(n)]
    assert e["pairs"] == n and close(e["mean"], float(np.mean(d)), 1e-12)
    assert close(e["stderr"], float(np.std(d, ddof=1) / math.sqrt(n)))
    assert isinstance(slab, T.SlabSummary)


# ------------------------------------------------------------------ the package's host path
def test_summarize_host_equals_the_restatement(case):
    from dexterous_rl_manipulation_amd import training_study as T

    class S:  # what native_specs builds, without loading the library
        def __init__(self, t):
            self.col, self.x_col, self.window, self.threshold, self.final_window = t

    got = T.summarize_host(case["tables"], K.RUN_ROWS, [S(t) for t in K.SPECS], case["off"], case["flat"], K.CONTRASTS)
    for a, b in zip(got[:3], case["out"][:3]):
        assert a.tobytes() == b.tobytes()
    assert got[3] == case["out"][3]
    off, flat = K.csr({"bad": [K.CRAFTED, K.R, -1, K.NEVER], "good": [K.CRAFTED, K.NEVER]})
    rows = K.RUN_ROWS.copy()
    rows[K.ONE] = K.CAP + 1
    got = T.summarize_host(case["tables"], rows, [S(t) for t in K.SPECS], off, flat, [[1.0, -1.0]])
    want = P.summarize(case["tables"], rows, K.SPECS, off, flat, [[1.0, -1.0]])
    for a, b in zip(got[:3], want[:3]):
        assert a.tobytes() == b.tobytes()
    assert got[3] == want[3] == P.ST_RANGE | P.ST_ROWS | P.ST_CONTRAST  # the two groups differ in size


# ------------------------------------------------------------------ a synthetic StudyResult
def synthetic_result(tables, seeds=(42, 123, 456)):
    """The four ablation arms x three seeds on twelve crafted runs (the slab's runs, twice), both
    slabs summarised by the restatement."""
    from dexterous_rl_manipulation_amd import training_study as T
    arms = [a.name for a in A.pg_component_arms()]
    order = [K.CRAFTED, K.EXACT_W, K.NEVER, K.EXACT_W, K.ONE, K.CRAFTED, K.NEVER, K.SHORT, K.CRAFTED, K.ONE, K.NEVER,
             K.EXACT_W]
    t, rows = tables[order][:, :, :16], K.RUN_ROWS[order]
    specs = A.pg_study_specs(window=K.W, threshold=K.THR, final_window=3)
    names = T._SLAB_COLUMNS["validation"]
    tuples = [(names.index(s.column), names.index(s.x_column), s.window, s.threshold, s.final_window) for s in specs]
    groups = {a: [i * len(seeds) + k for k in range(len(seeds))] for i, a in enumerate(arms)}
    off, flat = K.csr(groups)
    w = T.contrast_matrix(arms, A.PG_COMPONENT_CONTRASTS)
    rt, gt, ct, st = P.summarize(t, rows, tuples, off, flat, w)
    run_names = [(a, s) for a in arms for s in seeds]
    slab = lambda name: T.SlabSummary(name, specs, run_names, arms, list(A.PG_COMPONENT_CONTRASTS), rt, gt, ct, st)  # noqa: E731
    result = T.StudyResult(arms, seeds, 130, slab("training"), slab("validation"), A.PG_COMPONENT_CONTRASTS,
                           [3, 2, 3] + [None] * 3 + [1, 1, 0] + [None] * 3, [0] * 12, bytes_copied=1234)
    return result, rt


def test_report_json_and_accessors_of_a_synthetic_study(case, capsys, tmp_path):
    from dexterous_rl_manipulation_amd import pg_ablation, training_study as T
    result, rt = synthetic_result(case["tables"])
    assert result.run_index("no_curriculum", 123) == 4 and result.yardstick is result.validation
    assert result.validation.run("success_rate", "convergence_row").tolist() == rt[:, 0, P.CONV].tolist()
    g = result.training.group("baseline", "success_rate", "final_window_mean")
    assert list(g) == list(T.GROUP_COLUMNS) and g["count"] == 3
    with pytest.raises(KeyError, match="no spec"):
        result.training.group("baseline", "value_mse", "best")
    stats = A.pg_statistics(result)
    A.print_ablation_report({}, stats)
    out = capsys.readouterr().out
    assert "Component Ablation Report" in out and "No Curriculum:" in out and "Minimal:" in out
    assert "Effects" not in out  # the effects entry is not a configuration
    # the same text as the report of the arms alone
    A.print_ablation_report({}, {k: v for k, v in stats.items() if k != "effects"})
    assert capsys.readouterr().out == out
    lines = pg_ablation.effect_lines(stats)
    assert len(lines) == 1 + len(A.PG_COMPONENT_CONTRASTS) and "interaction" in lines[3]
    path = tmp_path / "study.json"
    result.save(path)
    d = json.loads(path.read_text())  # standard JSON: NaN travels as a string
    assert d["format"] == T.STUDY_FORMAT and d["arms"] == result.arms and d["seeds"] == [42, 123, 456]
    assert d["progression_steps"][:4] == [3, 2, 3, None] and d["bytes_copied"] == 1234
    back = np.array([[[float(x) for x in s] for s in r] for r in d["validation"]["run_table"]])
    assert np.array_equal(back, rt, equal_nan=True)
    assert d["validation"]["specs"][0] == {"column": "success_rate", "x_column": "env_steps", "window": K.W,
                                           "threshold": K.THR, "final_window": 3}
    whole = pg_ablation.results_json(stats, result)
    json.dumps(whole, allow_nan=False)
    assert set(whole) == {"statistics", "study"} and set(whole["statistics"]) == set(stats)
    agg = CA.pg_aggregates(T.StudyResult(result.arms[:2], result.seeds, 130, result.training, None,
                                         {"no_curriculum_vs_baseline": {}}))
    assert set(agg) == {"baseline", "no_curriculum", "effects"}
    assert set(agg["baseline"]["aggregated_metrics"]) == set(CA._PG_AGGREGATES) | {"num_converged"}


def test_runner_rejects_bad_arguments_before_building_anything():
    from dexterous_rl_manipulation_amd import training_study as T
    arm = T.Arm("x", False, "dense")
    for kw, msg in ((dict(arms=[], seeds=[1], iterations=1), "at least one arm"),
                    (dict(arms=[arm, arm], seeds=[1], iterations=1), "distinct"),
                    (dict(arms=[arm], seeds=[1, 1], iterations=1), "distinct"),
                    (dict(arms=[arm], seeds=[1], iterations=0), "at least one"),
                    (dict(arms=[arm], seeds=[1], iterations=1, validate_every=-1), "validate_every"),
                    (dict(arms=[arm], seeds=[1], iterations=1, train_specs=[T.Spec("nope")]), "column"),
                    (dict(arms=[arm], seeds=[1], iterations=1, train_specs=[T.Spec("success_rate", window=0)]), "window"),
                    (dict(arms=[arm], seeds=[1], iterations=1, val_specs=[]), "specs"),
                    (dict(arms=[arm], seeds=[1], iterations=1, contrasts={"c": {"y": 1.0}}), "not an arm")):
        with pytest.raises(ValueError, match=msg):
            T.run_training_study(**kw)


def test_command_arguments():
    from dexterous_rl_manipulation_amd import pg_ablation
    a = pg_ablation.parse_args(["--iterations", "3", "--envs", "128", "--horizon", "16"])
    kw = pg_ablation.study_arguments(a)
    assert (kw["iterations"], kw["num_envs"], kw["horizon"]) == (3, 128, 16)
    assert kw["seeds"] == [42, 123, 456, 789, 1000] and kw["max_steps"] == 200 and kw["output_dir"] == "logs"
    assert kw["validate_every"] == 10 and kw["val_episodes"] == 5 and kw["device_summary"] is True
    assert kw["curriculum_scheduler_config"].window_size == 15
    a = pg_ablation.parse_args(["--config-name", "quick_test", "--iterations", "5", "--seeds", "7", "8", "--out", "o",
                                "--host-summary", "--validate-every", "2", "--val-episodes", "3"])
    kw = pg_ablation.study_arguments(a)
    assert kw["seeds"] == [7, 8] and kw["output_dir"] == "o" and kw["device_summary"] is False
    assert kw["max_steps"] == 100 and kw["curriculum_scheduler_config"].progression_steps == 3
    assert (kw["validate_every"], kw["val_episodes"]) == (2, 3)
    assert pg_ablation.study_arguments(pg_ablation.parse_args(["--config-name", "quick_test", "--iterations", "1"]))[
        "seeds"] == [42, 123]
    for bad in (["--envs", "8"], ["--iterations", "0"], ["--iterations", "2", "--validate-every", "-1"],
                ["--iterations", "2", "--config", "a.json", "--config-name", "default"]):
        with pytest.raises(SystemExit):
            pg_ablation.parse_args(bad)


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def native():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        d.build.build_native()
    return _native


def test_struct_layout_and_constants_match_c(native):
    """dxrl_pg_runs_args / dxrl_pg_runs_spec and the table constants against their ctypes mirrors,
    by a gcc-compiled probe."""
    structs = (("dxrl_pg_runs_args", native.PgRunsArgs), ("dxrl_pg_runs_spec", native.PgRunsSpec))
    consts = {"abi": "DXRL_ABI_VERSION", "max_specs": "DXRL_PG_RUNS_MAX_SPECS", "run_cols": "DXRL_PG_RUNS_RUN_COLS",
              "metrics": "DXRL_PG_RUNS_METRICS", "group_cols": "DXRL_PG_RUNS_GROUP_COLS",
              "contrast_cols": "DXRL_PG_RUNS_CONTRAST_COLS", "log_cols": "DXRL_PG_LOG_COLS",
              "val_cols": "DXRL_PG_VAL_COLS", "last_run_col": "DXRL_PG_RUNS_RUN_NAN_ROWS",
              "last_metric": "DXRL_PG_RUNS_CURVE_MEAN", "conv_col": "DXRL_PG_RUNS_RUN_CONVERGENCE_ROW",
              "conv_metric": "DXRL_PG_RUNS_CONVERGENCE_ROW"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    lines += [f'printf("{k} %d\\n", (int){v});' for k, v in consts.items()]
    for s, mirror in structs:
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f, _ in mirror._fields_]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {k: int(v) for k, v in (line.split() for line in out if line)}
    for s, mirror in structs:
        assert got[s] == C.sizeof(mirror)
        for f, _ in mirror._fields_:
            assert got[f"{s}.{f}"] == getattr(mirror, f).offset, (s, f)
    assert got["abi"] == native.ABI_VERSION == 1
    assert got["max_specs"] == native.PG_RUNS_MAX_SPECS
    assert got["run_cols"] == native.PG_RUNS_RUN_COLS == len(native.PG_RUNS_RUN_COLUMNS) == P.RUN_COLS
    assert got["metrics"] == len(native.PG_RUNS_METRICS) == P.METRICS
    assert got["group_cols"] == len(native.PG_RUNS_GROUP_COLUMNS) == P.GROUP_COLS
    assert got["contrast_cols"] == len(native.PG_RUNS_CONTRAST_COLUMNS) == P.CONTRAST_COLS
    assert (got["log_cols"], got["val_cols"]) == (native.PG_LOG_COLS, native.PG_VAL_COLS) == (24, 16)
    assert got["last_run_col"] == native.PG_RUNS_RUN_COLUMNS.index("nan_rows") == P.NAN_ROWS
    assert got["last_metric"] == native.PG_RUNS_METRICS.index("curve_mean") == P.M_CURVE
    assert got["conv_col"] == native.PG_RUNS_RUN_COLUMNS.index("convergence_row") == P.CONV
    assert got["conv_metric"] == native.PG_RUNS_METRICS.index("convergence_row") == P.M_CONV
    assert [native.PG_RUNS_RUN_COLUMNS.index(m) for m in native.PG_RUNS_METRICS] == list(P.METRIC_RUN_COL)
    assert (native.PG_RUNS_ST_RANGE, native.PG_RUNS_ST_ROWS, native.PG_RUNS_ST_CONTRAST) == \
        (P.ST_RANGE, P.ST_ROWS, P.ST_CONTRAST)


def test_entry_rejects_bad_arguments_before_any_launch(native):
    a = native.PgRunsArgs()
    specs = (native.PgRunsSpec * 2)()
    fake = 1 << 20  # never dereferenced: the checks run first
    with pytest.raises(ValueError, match="null args"):
        native.call("dxrl_pg_runs_summarize", 0, None, None)

    def fill():
        a.num_runs, a.cap, a.cols, a.num_specs, a.num_groups, a.num_members, a.num_contrasts = 6, 130, 24, 2, 3, 5, 2
        for s in specs:
            s.col, s.x_col, s.window, s.final_window, s.threshold = 5, 1, 4, 10, 0.5
        a.specs = specs
        for k in ("tables", "run_rows", "group_offsets", "group_runs", "contrast_weights", "run_table", "group_table",
                  "contrast_table", "status"):
            setattr(a, k, fake)

    def rejected(msg):
        with pytest.raises(ValueError, match=msg):
            native.call("dxrl_pg_runs_summarize", 0, C.byref(a), None)

    for field, value, msg in (("num_runs", 0, "num_runs"), ("cap", 0, "cap"), ("cols", 0, "cols"),
                              ("num_specs", 0, "num_specs"), ("num_specs", native.PG_RUNS_MAX_SPECS + 1, "num_specs"),
                              ("num_groups", -1, "num_groups"), ("num_contrasts", -1, "num_contrasts"),
                              ("num_members", -1, "num_members"), ("num_groups", 0, "no group"),
                              ("tables", None, "null tables"), ("run_rows", None, "run_rows"),
                              ("run_table", None, "run_table"), ("status", None, "status"),
                              ("group_offsets", None, "group_offsets"), ("group_runs", None, "group_runs"),
                              ("group_table", None, "group_table"), ("contrast_weights", None, "contrast_weights"),
                              ("contrast_table", None, "contrast_table")):
        fill()
        setattr(a, field, value)
        rejected(msg)
    fill()
    a.specs = C.POINTER(native.PgRunsSpec)()
    rejected("specs")
    for field, value, msg in (("col", -1, "col"), ("col", 24, "col"), ("x_col", -1, "x_col"), ("x_col", 24, "x_col"),
                              ("window", 0, "window"), ("final_window", 0, "final_window")):
        fill()
        setattr(specs[1], field, value)
        rejected(msg)
    fill()  # cols is the bound: column 16 of a validation table does not exist
    a.cols = 16
    specs[0].col = 16
    rejected("outside the 16 columns")
