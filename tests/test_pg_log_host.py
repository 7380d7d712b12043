"""CPU checks of the training-run layer: the NumPy restatement of the log row / header / window
rules (tests/pg_log_reference.py) on hand-computed cases and against a literal transcription of
the reference's convergence loop, TrainingLog and checkpoint files, the schedulers' state round
trip, the C ABI of dxrl_pg_log_row, and the CLI's arguments."""
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from dexterous_rl_manipulation_amd import experiments as X

import pg_log_reference as L

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


# ------------------------------------------------------------------ the restatement, by hand
def tiny(**kw):
    """n = 2, T = 2: every number below is computed by hand."""
    a = dict(n=2, T=2, iteration=7, env_steps=44, ep_count=[1, 2], ep_sum_return=[1.5, 4.5], ep_sum_length=[3, 6],
             ep_successes=[0, 1], rew=[1.0, 2.0, 3.0, 6.0], ret=[1.0, 3.0, 5.0, 7.0], done=[0, 1, 0, 255],
             values=[0.0, 1.0, 6.0, 9.0, 1e30, 1e30], stats=[4, 0, 0.25, 0, 2.0, 0, 0, 0],
             loss_partial=[[1.0, 2.0, 3.0, 4.0], [3.0, 2.0, 1.0, 0.0]], loss_rows=4, gnorm2=9.0)
    a.update(kw)
    return L.row_values(**a)


def test_row_by_hand():
    v = tiny()
    assert (v["iteration"], v["env_steps"], v["episodes"]) == (7.0, 44.0, 3.0)
    assert v["mean_return"] == 2.0 and v["mean_length"] == 3.0 and v["success_rate"] == 1 / 3
    assert v["mean_step_reward"] == 3.0 and v["done_fraction"] == 0.5
    assert v["value_mean"] == 4.0  # the 1e30 bootstrap slots are not read
    assert v["target_mean"] == 4.0 and v["target_var"] == 5.0  # deviations -3 -1 1 3
    # residuals 1 2 -1 -2: mean 0, variance 2.5
    assert v["residual_var"] == 2.5 and v["explained_variance"] == 0.5
    assert (v["adv_mean"], v["adv_std"]) == (0.25, 2.0)
    assert (v["policy_loss"], v["value_mse"], v["clip_frac"], v["approx_kl"]) == (1.0, 1.0, 1.0, 1.0)
    assert v["grad_norm"] == 3.0


def test_nan_rules():
    v = tiny(ep_count=[0, 0])
    assert v["episodes"] == 0.0
    assert all(math.isnan(v[k]) for k in ("mean_return", "mean_length", "success_rate"))
    v = tiny(ret=[2.0, 2.0, 2.0, 2.0])
    assert v["target_var"] == 0.0 and math.isnan(v["explained_variance"])
    assert v["residual_var"] > 0.0


def test_keep_best_tie_nan_and_gate():
    nan = float("nan")
    #          row: 0    1    2    3    4    5    6
    scores = [1.0, 3.0, 3.0, nan, 9.0, 4.0, 2.0]
    episodes = [5, 5, 5, 5, 1, 5, 0]  # row 4 is below min_episodes = 2
    best, header, table = L.series_rules(scores, episodes, 2, [0.0] * 7, 1, 1e9)
    assert best == [0, 1, 5]  # the tie at row 2 does not replace row 1; NaN and the gated 9.0 never win
    assert header["best_row"] == 5 and header["best_score"] == 4.0 and header["rows_written"] == 7
    assert table[:, L.IS_BEST].tolist() == [1, 1, 0, 0, 0, 1, 0]
    # off: score_col < 0 sets nothing
    t, h = np.zeros((1, L.COLS)), L.new_header()
    assert not L.finish_row(t, h, 0, {"episodes": 3.0, "mean_return": 1.0})
    assert h["best_row"] == -1 and h["best_score"] == -math.inf


def reference_convergence_step(rewards, window, threshold):
    """training/reward_comparison.py:113-124, transcribed."""
    episode_rewards = []
    convergence_step = None
    for episode in range(len(rewards)):
        episode_rewards.append(rewards[episode])
        if convergence_step is None and len(episode_rewards) >= window:
            recent_avg = np.mean(episode_rewards[-window:])
            if recent_avg > threshold:
                convergence_step = episode - window + 1
    return convergence_step


# a recorded series of mean episode returns per row: slow start, a dip, then over the threshold
SERIES = [0.11, 0.18, 0.32, 0.27, 0.41, 0.38, 0.52, 0.49, 0.61, 0.58, 0.44, 0.66, 0.71, 0.69, 0.75, 0.62]


@pytest.mark.parametrize("window,threshold", [(1, 0.5), (3, 0.5), (4, 0.55), (5, 0.6), (10, 0.5), (16, 0.4), (3, 5.0)])
def test_window_rule_equals_the_reference_loop(window, threshold):
    _, header, table = L.series_rules([0.0] * len(SERIES), [1] * len(SERIES), 1, SERIES, window, threshold)
    want = reference_convergence_step(SERIES, window, threshold)
    got = None if header["converged_row"] < 0 else header["converged_row"] - window + 1
    assert got == want
    wm = table[:, L.IDX["window_mean"]]
    assert np.all(np.isnan(wm[:window - 1])) and not np.any(np.isnan(wm[window - 1:]))
    for r in range(window - 1, len(SERIES)):
        assert wm[r] == pytest.approx(np.mean(SERIES[r - window + 1:r + 1]), rel=1e-15)


def test_window_rule_is_strict_sticks_and_ignores_nan():
    # means of window 2: -, 1.0, 2.0 (== threshold: no), 2.5 (first crossing), 0.5, 3.0
    vals = [1.0, 1.0, 3.0, 2.0, -1.0, 7.0]
    _, header, _ = L.series_rules([0.0] * 6, [1] * 6, 1, vals, 2, 2.0)
    assert header["converged_row"] == 3
    # a NaN in the window never converges; the first clean window does
    vals = [9.0, float("nan"), 9.0, 9.0]
    _, header, table = L.series_rules([0.0] * 4, [1] * 4, 1, vals, 2, 1.0)
    assert header["converged_row"] == 3 and np.isnan(table[1:3, L.IDX["window_mean"]]).all()


# ------------------------------------------------------------------ TrainingLog
def fake_log(run, rows=5, window=2):
    t = np.zeros((rows, L.COLS))
    t[:, 0] = np.arange(10, 10 + rows)
    t[:, 1] = 32 * (np.arange(rows) + 1)
    t[:, 2] = [0, 3, 4, 2, 5][:rows]
    t[:, L.IDX["mean_return"]] = [np.nan, 0.1 + 0.2, 1 / 3, -2.5e-7, 0.75][:rows]
    t[:, L.IDX["window_mean"]] = np.nan
    header = {"rows_written": rows, "best_row": 4, "converged_row": 3, "best_score": 0.75}
    return run.TrainingLog(t, header, window, {"keep_best": "mean_return"})


def test_training_log_columns_and_json_round_trip(run, tmp_path):
    assert run.COLUMNS == L.COLUMNS and run.COLS == L.COLS
    log = fake_log(run)
    assert len(log) == 5 and set(log.columns) == set(L.COLUMNS)
    assert log.best_iteration == 14 and log.convergence_iteration == 12  # rows 4 and 3 - 2 + 1
    p = tmp_path / "log.json"
    log.save(p)
    json.loads(p.read_text())  # standard JSON: no bare NaN tokens
    assert "NaN" not in p.read_text()
    back = run.TrainingLog.load(p)
    assert back.table.tobytes() == log.table.tobytes()  # bit for bit, NaN included
    assert back.header == log.header and back.window == 2 and back.settings == log.settings
    st = back.statistics()
    assert st["iterations"] == 5 and st["episodes"] == 14 and st["env_steps"] == 160
    assert st["best_iteration"] == 14 and st["max_mean_return"] == 0.75 and st["final_mean_return"] == 0.75
    empty = run.TrainingLog(np.zeros((0, L.COLS)), L.new_header(), None)
    assert empty.best_iteration is None and empty.convergence_iteration is None
    assert run.TrainingLog.from_dict(json.loads(json.dumps(empty.to_dict()))).header["best_score"] == -math.inf
    with pytest.raises(ValueError):
        run.TrainingLog.from_dict({"format": "other"})


# ------------------------------------------------------------------ schedulers
def feed(sc, rng, episodes):
    ok = rng.random(episodes) < 0.8
    steps = rng.integers(5, 60, episodes)
    for a, b in zip(ok, steps):
        sc.update(bool(a), int(b))


def make_sched(kind, history):
    a, b = X.CurriculumConfig.easy(), X.CurriculumConfig.hard()
    if kind == "window":
        return X.CurriculumScheduler(a, b, success_rate_threshold=0.6, min_episodes_before_progression=10,
                                     window_size=8, progression_steps=50, history=history)
    return X.StepBasedScheduler(a, b, [300, 900, 2000, 4000], window_size=8, history=history)


@pytest.mark.parametrize("kind", ["window", "steps"])
@pytest.mark.parametrize("history", ["full", "window"])
def test_scheduler_state_round_trip_mid_progression(kind, history):
    one, two = make_sched(kind, history), make_sched(kind, history)
    feed(one, np.random.default_rng(5), 40)
    feed(two, np.random.default_rng(5), 40)
    assert 0.0 < one.get_difficulty_level() < 1.0  # in the middle of the progression
    state = json.loads(json.dumps(one.get_state()))  # JSON-able
    back = X.scheduler_from_state(state)
    assert type(back) is type(one) and back.get_state() == one.get_state()
    cur, want = back.get_current_config(), one.get_current_config()
    assert cur == want
    # numpy scalars survive (a numpy.float64 friction changes the env step's arithmetic)
    assert type(cur.friction_coefficient) is type(want.friction_coefficient)
    assert bytes(cur.to_native()) == bytes(want.to_native())
    # both continue identically
    feed(back, np.random.default_rng(6), 60)
    feed(two, np.random.default_rng(6), 60)
    assert back.get_state() == two.get_state() and back.get_statistics() == two.get_statistics()
    assert len(back.progression_history) > len(one.progression_history)
    with pytest.raises(ValueError):
        make_sched("steps" if kind == "window" else "window", history).set_state(state)


def test_curriculum_config_state_keeps_numpy_scalars():
    c = X.CurriculumConfig(friction_coefficient=np.float64(0.4), object_size_range=(0.03, 0.07))
    back = X.CurriculumConfig.from_state(json.loads(json.dumps(c.to_state())))
    assert back == c and isinstance(back.friction_coefficient, np.floating)
    assert not isinstance(back.object_mass, np.floating) and back.object_size_range == (0.03, 0.07)


# ------------------------------------------------------------------ checkpoint file
def test_checkpoint_file_round_trip(run, tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"params": rng.standard_normal(37).astype(np.float32), "packed": rng.integers(-2**15, 2**15, 11).astype(np.int16),
              "ep_ret": rng.standard_normal(5), "env_state": rng.integers(0, 256, 100).astype(np.uint8),
              "log_table": np.full((2, L.COLS), np.nan)}
    meta = {"step_count": 3, "iteration_index": 2, "scheduler": make_sched("window", "window").get_state(),
            "trainer_config": {"betas": [0.9, 0.999], "lr": 3e-4}}
    p = tmp_path / "ck.npz"
    run.write_checkpoint(p, arrays, meta)
    got, m = run.read_checkpoint(p)
    assert set(got) == set(arrays)
    for k in arrays:
        assert got[k].dtype == arrays[k].dtype and got[k].tobytes() == arrays[k].tobytes()
    assert m == dict(meta, format=run.CHECKPOINT_FORMAT)
    with np.load(p, allow_pickle=False) as z:  # no pickled objects inside
        assert all(z[k].dtype != object for k in z.files)
    other = tmp_path / "other.npz"
    np.savez(other, x=np.zeros(1))
    with pytest.raises(ValueError):
        run.read_checkpoint(other)


# ------------------------------------------------------------------ C ABI
def test_pg_log_struct_layouts_match_c(native):
    """dxrl_pg_log_args / dxrl_pg_log_header against their ctypes mirrors, by a gcc-compiled probe."""
    structs = (("dxrl_pg_log_args", native.PgLogArgs), ("dxrl_pg_log_header", native.PgLogHeader))
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("abi %d\\n", DXRL_ABI_VERSION);', 'printf("cols %d\\n", DXRL_PG_LOG_COLS);',
             'printf("named %d\\n", (int)DXRL_PG_LOG_NAMED);', 'printf("is_best %d\\n", (int)DXRL_PG_LOG_IS_BEST);',
             'printf("window_mean %d\\n", (int)DXRL_PG_LOG_WINDOW_MEAN);',
             'printf("grad_norm %d\\n", (int)DXRL_PG_LOG_GRAD_NORM);']
    for s, mirror in structs:
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
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
    for s, mirror in structs:
        assert int(got[s]) == C.sizeof(mirror)
        for f, _ in mirror._fields_:
            assert int(got[f"{s}.{f}"]) == getattr(mirror, f).offset, (s, f)
    assert int(got["abi"]) == native.ABI_VERSION == 1
    assert int(got["cols"]) == native.PG_LOG_COLS == L.COLS and L.COLS % 4 == 0
    assert int(got["named"]) == native.PG_LOG_NAMED == len(L.COLUMNS) <= L.COLS
    assert int(got["is_best"]) == native.PG_LOG_IS_BEST == L.IS_BEST
    assert int(got["window_mean"]) == L.IDX["window_mean"] and int(got["grad_norm"]) == L.IDX["grad_norm"]
    assert native.PG_LOG_COLUMNS == L.COLUMNS
    assert C.sizeof(native.PgLogHeader) == 64


# ------------------------------------------------------------------ CLI
def test_cli_arguments():
    from dexterous_rl_manipulation_amd import train
    a = train.parse_args(["--iterations", "3", "--out", "o"])
    assert (a.config_name, a.config, a.iterations, a.out, a.resume) == ("easy", None, 3, "o", None)
    assert a.keep_best == "mean_return" and a.converge is None and a.poll_every == 0
    a = train.parse_args(["--config-name", "default", "--iterations", "5", "--out", "o", "--resume", "c.npz",
                          "--keep-best", "success_rate", "--converge", "mean_return", "10", "0.5"])
    assert a.config_name == "default" and a.resume == "c.npz" and a.keep_best == "success_rate"
    assert a.converge == ("mean_return", 10, 0.5)
    assert train.parse_args(["--config", "f.json", "--iterations", "1", "--out", "o"]).config_name is None
    assert train.parse_args(["--iterations", "1", "--out", "o", "--keep-best", "none"]).keep_best is None
    for bad in (["--out", "o"], ["--iterations", "1"], ["--iterations", "-1", "--out", "o"],
                ["--iterations", "1", "--out", "o", "--config-name", "easy", "--config", "f.json"],
                ["--iterations", "1", "--out", "o", "--config-name", "nope"],
                ["--iterations", "1", "--out", "o", "--keep-best", "is_best"],
                ["--iterations", "1", "--out", "o", "--converge", "window_mean", "3", "0.5"],
                ["--iterations", "1", "--out", "o", "--converge", "mean_return", "0", "0.5"],
                ["--iterations", "1", "--out", "o", "--converge", "mean_return", "x", "0.5"],
                ["--iterations", "1", "--out", "o", "--stop-on-converge"]):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
