"""CPU checks of the paired validation layer (common random numbers across noise levels): the
NumPy restatement (tests/pg_val_paired_reference.py) by hand and against the direct two-pass
reduction on the GPU test's shapes and kinds, the layout of dxrl_pg_val_paired_args, its column
enum and the stream_period field against include/dxrl.h, every argument check of
dxrl_pg_val_paired_row (each returns before any launch, so no device is needed), ValidationLog
with and without the paired table through JSON and through a checkpoint's optional entries, the
fingerprint rule, and the CLI's arguments."""
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pg_val_paired_reference as P
import pg_val_reference as V
from test_pg_val_levels_host import NOISE, fake_levels_validation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dxrl.h")


@pytest.fixture(scope="module")
def native():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        d.build.build_native()
    return _native


@pytest.fixture(scope="module")
def run():
    from dexterous_rl_manipulation_amd import training_run
    return training_run


# ------------------------------------------------------------------ the restatement
def test_paired_row_by_hand():
    # 2 objects x 2 episodes; the level loses record 0 and 3, gains record 2
    ret = [1.0, 3.0, 5.0, 7.0, 0.0, 3.0, 9.0, 3.0]
    length = [10, 4, 6, 8, 12, 4, 2, 8]
    suc = [1, 255, 0, 1, 0, 7, 1, 0]
    rows, lost = P.paired_row(2, 2, 2, ret, length, suc)
    a, b = rows
    assert a == {"pairs": 4.0, "lost": 0.0, "gained": 0.0, "both_success": 3.0, "both_fail": 1.0,
                 "mean_return_diff": 0.0, "return_diff_std": 0.0, "return_diff_stderr": 0.0, "mean_length_diff": 0.0,
                 "paired_degradation": 0.0, "paired_degradation_stderr": 0.0, "mcnemar": 0.0,
                 "objects_with_loss": 0.0, "max_object_lost": 0.0}
    assert (b["lost"], b["gained"], b["both_success"], b["both_fail"]) == (2.0, 1.0, 1.0, 0.0)
    assert b["mean_return_diff"] == -0.25  # d = -1 0 4 -4
    assert b["return_diff_std"] == math.sqrt(32.75 / 4) and b["return_diff_stderr"] == math.sqrt(32.75 / 12)
    assert b["mean_length_diff"] == -0.5 and b["paired_degradation"] == 0.25
    assert b["paired_degradation_stderr"] == math.sqrt((3 - 0.25) / 4) / 2 and b["mcnemar"] == 1 / 3
    assert lost.tolist() == [[0, 0], [1, 1]] and b["objects_with_loss"] == 2.0 and b["max_object_lost"] == 1.0
    assert P.paired_array(rows).shape == (2, P.PAIRED_COLS) and lost.dtype == np.int32


def test_one_pair_has_no_standard_error():
    rows, lost = P.paired_row(2, 1, 1, [2.0, -1.0], [5, 9], [1, 0])
    for r in rows:
        assert math.isnan(r["return_diff_stderr"]) and r["return_diff_std"] == 0.0 and r["pairs"] == 1.0
    assert rows[1]["mean_return_diff"] == -3.0 and rows[1]["lost"] == 1.0 and rows[1]["mcnemar"] == 1.0
    assert rows[1]["paired_degradation"] == 1.0 and rows[1]["paired_degradation_stderr"] == 0.0
    assert rows[1]["mean_length_diff"] == 4.0 and lost.tolist() == [[0], [1]]


def test_the_derived_columns_never_leave_their_range():
    for n, lost, gained in ((1, 1, 0), (2 ** 31 - 1, 2 ** 31 - 1, 0), (3 * 2 ** 28 + 1, 0, 3 * 2 ** 28 + 1), (7, 3, 3)):
        d = P.derived(lost, gained, n)
        assert d["paired_degradation_stderr"] >= 0.0 and not math.isnan(d["paired_degradation_stderr"])
        assert d["paired_degradation"] == (lost - gained) / n
    assert P.derived(0, 0, 9) == {"paired_degradation": 0.0, "paired_degradation_stderr": 0.0, "mcnemar": 0.0}
    assert P.derived(3, 3, 7)["mcnemar"] == 0.0


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("L,G,K", P.SHAPES)
def test_restatement_against_the_two_pass_reduction(L, G, K, kind):
    d = P.records(L, G, K, kind, seed=L + G + K)
    rows, lost = P.paired_row(L, G, K, d["ep_return"], d["ep_length"], d["ep_success"])
    n = G * K
    s0 = d["ep_success"][:n] != 0
    for l, r in enumerate(rows):
        s = slice(l * n, (l + 1) * n)
        sl = d["ep_success"][s] != 0
        assert r["lost"] + r["gained"] + r["both_success"] + r["both_fail"] == r["pairs"] == n
        assert r["lost"] - r["gained"] == int(s0.sum()) - int(sl.sum())
        assert lost[l].sum() == r["lost"] and lost[l].max() == r["max_object_lost"]
        diff = d["ep_return"][s] - d["ep_return"][:n]
        mean, std, stderr = P.two_pass(d["ep_return"][:n], d["ep_return"][s])
        assert abs(r["mean_return_diff"] - mean) <= P.sum_bound(diff) / n
        for got, want in ((r["return_diff_std"], std), (r["return_diff_stderr"], stderr)):
            if math.isnan(want):
                assert n == 1 and math.isnan(got)
            elif want == 0.0:
                assert got == 0.0
            else:
                assert abs(got - want) <= 1e-9 * want
        assert r["mean_length_diff"] == float(d["ep_length"][s].astype(np.int64).sum()
                                              - d["ep_length"][:n].astype(np.int64).sum()) / n
        if l == 0 or kind == "all_pairs_equal":
            assert all(r[k] == 0.0 for k in P.PAIRED_COLUMNS[5:] if k != "return_diff_stderr" or n > 1)
        if kind == "every_success_lost" and l > 0:
            assert r["lost"] == s0.sum() > 0 and r["gained"] == 0 and r["mcnemar"] == r["lost"]
        if kind == "no_discordant_pair":
            assert r["lost"] == r["gained"] == r["mcnemar"] == r["paired_degradation_stderr"] == 0.0


# ------------------------------------------------------------------ C ABI
def test_paired_struct_layout_enum_and_stream_period_match_c(native):
    structs = dict(native.LATER_STRUCTS)
    s, mirror = "dxrl_pg_val_paired_args", structs["dxrl_pg_val_paired_args"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("cols %d\\n", DXRL_PG_VAL_PAIRED_COLS);', 'printf("named %d\\n", (int)DXRL_PG_VAL_PAIRED_NAMED);',
             f'printf("{s} %zu\\n", sizeof({s}));', 'printf("eval %zu\\n", sizeof(dxrl_eval_args));',
             'printf("period %zu\\n", offsetof(dxrl_eval_args, stream_period));']
    enum = {"paired_degradation": "DEGRADATION", "paired_degradation_stderr": "DEGRADATION_STDERR"}
    for name in P.PAIRED_COLUMNS:
        lines.append(f'printf("P.{name} %d\\n", (int)DXRL_PG_VAL_PAIRED_{enum.get(name, name.upper())});')
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
    assert int(got["cols"]) == int(got["named"]) == native.PG_VAL_PAIRED_COLS == P.PAIRED_COLS == 14
    assert native.PG_VAL_PAIRED_COLUMNS == P.PAIRED_COLUMNS
    for name in P.PAIRED_COLUMNS:
        assert int(got[f"P.{name}"]) == P.PIDX[name]
    # the period of the episode arguments: behind the three stream keys it addresses
    assert int(got["eval"]) == C.sizeof(native.EvalArgs)
    assert int(got["period"]) == native.EvalArgs.stream_period.offset == native.EvalArgs.reset_seed.offset + 8
    names = [f for f, _ in native.EvalArgs._fields_]
    assert names[names.index("reset_seed") + 1] == "stream_period" and native.EvalArgs().stream_period == 0
    for fn in ("dxrl_pg_val_paired_row", "dxrl_pg_val_paired_partial_doubles"):
        assert fn in native._SIGS and fn in open(HEADER).read()


def good_args(native):
    """Arguments that pass every check; the pointers are never dereferenced on the host."""
    fake = 1 << 20
    a = native.PgValPairedArgs()
    a.num_levels, a.num_objects, a.episodes_per_object, a.row, a.cap = 4, 3, 5, 0, 4
    nb = C.c_int64()
    native.call("dxrl_pg_val_paired_partial_doubles", 4, 3, 5, C.byref(nb))
    a.partial_doubles = nb.value
    for k, name in enumerate(("ep_return", "ep_length", "ep_success", "partial", "paired", "object_lost")):
        setattr(a, name, fake + 4096 * k)
    return a


BAD = [
    ("num_levels", dict(num_levels=0)), ("num_levels", dict(num_levels=17)), ("num_levels", dict(num_levels=-2)),
    ("num_objects", dict(num_objects=0)), ("num_objects", dict(episodes_per_object=0)),
    ("num_objects", dict(num_objects=-3)),
    ("INT32_MAX", dict(num_objects=1 << 16, episodes_per_object=1 << 15)),
    ("INT32_MAX", dict(num_objects=2, episodes_per_object=1 << 62)),
    ("INT32_MAX", dict(num_levels=4, num_objects=1 << 15, episodes_per_object=1 << 14)),
    ("outside the table", dict(row=-1)), ("outside the table", dict(row=4)), ("outside the table", dict(cap=0)),
    ("null episode records", dict(ep_return=None)), ("null episode records", dict(ep_length=None)),
    ("null episode records", dict(ep_success=None)),
    ("null partial", dict(partial=None)), ("null partial", dict(paired=None)),
    ("partial holds", dict(partial_doubles=8)),
    ("partial holds", dict(partial_doubles=3 * (64 * 8 + 2))),  # room for three of the four levels
]


@pytest.mark.parametrize("match,change", BAD, ids=[f"{m.split()[0]}-{'-'.join(c)}-{i}" for i, (m, c) in enumerate(BAD)])
def test_paired_row_rejects_bad_arguments_before_any_launch(native, match, change):
    a = good_args(native)
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(ValueError, match=match):
        native.call("dxrl_pg_val_paired_row", 0, C.byref(a), None)


def test_paired_null_args_and_size_query(native):
    with pytest.raises(ValueError, match="null args"):
        native.call("dxrl_pg_val_paired_row", 0, None, None)
    nb, one = C.c_int64(), C.c_int64()
    for L, G, K in ((1, 1, 1), (2, 3, 5), (16, 256, 1), (3, 37, 33), (11, 64, 10)):
        native.call("dxrl_pg_val_paired_partial_doubles", L, G, K, C.byref(nb))
        native.call("dxrl_pg_val_levels_partial_doubles", L, G, K, C.byref(one))
        assert nb.value == one.value == L * (64 * 8 + (G + 1) // 2)  # a scratch of the levels row's size, its own
    for L, G, K in ((0, 1, 1), (17, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1 << 20, 1 << 20), (16, 1 << 14, 1 << 14)):
        with pytest.raises(ValueError):
            native.call("dxrl_pg_val_paired_partial_doubles", L, G, K, C.byref(nb))
    with pytest.raises(ValueError, match="null out"):
        native.call("dxrl_pg_val_paired_partial_doubles", 1, 1, 1, None)


# ------------------------------------------------------------------ ValidationLog
def fake_paired_validation(run, rows=3, G=2):
    """test_pg_val_levels_host.py's levels log with a paired table and per-object lost counts."""
    base = fake_levels_validation(run, rows, G)
    L = len(NOISE)
    paired = np.zeros((rows, L, P.PAIRED_COLS))
    lost = np.zeros((rows, L, G), dtype=np.int32)
    for r in range(rows):
        d = P.records(L, G, 3, "random", seed=r)
        lv, lost[r] = P.paired_row(L, G, 3, d["ep_return"], d["ep_length"], d["ep_success"])
        paired[r] = P.paired_array(lv)
    paired[0, 1, P.PIDX["return_diff_stderr"]] = np.nan  # a NaN must survive the round trip
    return run.ValidationLog(base.table, base.header, base.object_successes, base.object_names, base.settings,
                             noise_levels=NOISE, levels=base.levels, robust=base.robust, paired=paired,
                             object_lost=lost)


def test_validation_log_with_the_paired_table_and_its_json_round_trip(run, tmp_path):
    assert run.VAL_PAIRED_COLUMNS == P.PAIRED_COLUMNS and run.VAL_PAIRED_COLS == P.PAIRED_COLS
    val = fake_paired_validation(run)
    assert val.paired.shape == (3, 3, 14) and val.object_lost.shape == (3, 3, 2) and val.object_lost.dtype == np.int32
    assert val.paired_column("lost").shape == (3, 3) and np.all(val.paired_column("lost")[:, 0] == 0.0)
    st = val.statistics()
    assert st["common_random_numbers"] is True
    assert st["final_max_lost"] == val.paired_column("lost")[-1, 1:].max()
    assert st["final_min_mean_return_diff"] == val.paired_column("mean_return_diff")[-1, 1:].min()
    header = {"rows_written": 2, "best_row": 0, "converged_row": -1, "best_score": 0.5}
    log = run.TrainingLog(np.zeros((2, 24)), header, None, {"keep_best": "mean_return"}, validation=val)
    p = tmp_path / "log.json"
    log.save(p)
    text = p.read_text()
    d = json.loads(text)
    assert "NaN" not in text and d["validation"]["paired_columns"] == list(P.PAIRED_COLUMNS)
    bv = run.TrainingLog.load(p).validation
    assert bv.paired.tobytes() == val.paired.tobytes()  # NaN included
    assert bv.object_lost.dtype == np.int32 and np.array_equal(bv.object_lost, val.object_lost)
    assert bv.levels.tobytes() == val.levels.tobytes() and bv.robust.tobytes() == val.robust.tobytes()
    assert bv.table.tobytes() == val.table.tobytes() and bv.header == val.header and bv.settings == val.settings
    with pytest.raises(ValueError):
        run.ValidationLog.from_dict(dict(d["validation"], paired_columns=["other"]))


def test_logs_without_the_paired_table_serialise_as_before_and_old_json_loads(run):
    levels = fake_levels_validation(run)
    d = levels.to_dict()
    assert set(d) == {"columns", "settings", "object_names", "header", "rows", "object_successes", "noise_levels",
                      "level_columns", "robust_columns", "levels", "robust"}  # no new key
    assert levels.paired is None and levels.object_lost is None
    assert "common_random_numbers" not in levels.statistics() and "final_max_lost" not in levels.statistics()
    with pytest.raises(ValueError, match="common_random_numbers"):
        levels.paired_column("lost")
    back = run.ValidationLog.from_dict(json.loads(json.dumps(d)))  # a file the parent commit wrote
    assert back.paired is None and back.object_lost is None and back.levels.tobytes() == levels.levels.tobytes()
    t = np.zeros((2, V.COLS))
    header = {"rows_written": 2, "best_row": 1, "stopped_row": -1, "since_best": 0, "best_score": 0.5}
    plain = run.ValidationLog(t, header, np.arange(6, dtype=np.int32).reshape(2, 3), ["a", "b", "c"], {"patience": 0})
    assert set(plain.to_dict()) == {"columns", "settings", "object_names", "header", "rows", "object_successes"}
    assert plain.paired is None and "common_random_numbers" not in plain.statistics()
    with pytest.raises(ValueError, match="common_random_numbers"):
        plain.paired_column("lost")


def test_checkpoint_entries_with_the_paired_table_and_an_older_checkpoint(run, tmp_path):
    val = fake_paired_validation(run)
    old_fp = {"objects": [{"object_size": 0.07}], "episodes_per_object": 3, "seed": 0, "device_seed": 0,
              "max_steps": 12, "deterministic": True, "solve_threshold": 1.0, "reward_type": "dense",
              "noise_levels": [list(x) for x in NOISE]}
    fingerprint = dict(old_fp, common_random_numbers=True)
    raw_header = np.zeros(64, np.uint8)
    raw_header[:32].view(np.int64)[:] = [3, 1, -1, 1]
    raw_header[32:40].view(np.float64)[:] = 0.5
    best = np.arange(5, dtype=np.float32)
    arrays = run.validation_arrays(val.table, raw_header, best, val.object_successes, val.levels, val.robust,
                                   val.paired, val.object_lost)
    assert set(arrays) == {"val_table", "val_header", "val_best_params", "val_objects", "val_levels", "val_robust",
                           "val_paired", "val_object_lost"}
    p = tmp_path / "ck.npz"
    run.write_checkpoint(p, arrays, {"log": {"rows": 2},
                                     "validation": run.validation_meta(3, fingerprint, val.object_names, val.settings)})
    got, m = run.read_checkpoint(p)
    back = run.validation_log_of_checkpoint(got, m)
    assert back.paired.tobytes() == val.paired.tobytes() and np.array_equal(back.object_lost, val.object_lost)
    assert back.levels.tobytes() == val.levels.tobytes() and back.header == val.header
    # written before this change: no paired entries, a fingerprint without the key
    old = run.validation_arrays(val.table, raw_header, best, val.object_successes, val.levels, val.robust)
    assert set(old) == {"val_table", "val_header", "val_best_params", "val_objects", "val_levels", "val_robust"}
    q = tmp_path / "old.npz"
    run.write_checkpoint(q, old, {"log": {"rows": 2}, "validation": run.validation_meta(3, old_fp, val.object_names, {})})
    got, m = run.read_checkpoint(q)
    back = run.validation_log_of_checkpoint(got, m)
    assert back.paired is None and back.object_lost is None and back.levels.tobytes() == val.levels.tobytes()
    # the fingerprint rule: the key is there only when set, and a difference names it
    assert run.fingerprint_diff(old_fp, fingerprint) == ["common_random_numbers"]
    assert run.fingerprint_diff(fingerprint, dict(fingerprint)) == []


# ------------------------------------------------------------------ CLI
def test_cli_common_random_numbers_argument():
    from dexterous_rl_manipulation_amd import train
    base = ["--iterations", "1", "--out", "o"]
    a = train.parse_args(base + ["--validate-every", "1", "--val-obs-noise", "0.05"])
    assert a.val_common_random_numbers is False
    a = train.parse_args(base + ["--validate-every", "2", "--val-obs-noise", "0", "0.05", "--val-dyn-noise", "0.1",
                                 "--val-common-random-numbers"])
    assert a.val_common_random_numbers is True and len(a.val_noise_levels) == 4
    for bad in (["--val-common-random-numbers"],                              # no validation at all
                ["--validate-every", "1", "--val-common-random-numbers"],     # no noise levels
                ["--val-obs-noise", "0.1", "--val-common-random-numbers"]):   # no --validate-every
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)
