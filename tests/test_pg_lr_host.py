"""CPU checks of the step-size control layer: the schedules, the pure-Python restatement of the
device controller (tests/pg_lr_reference.py) on hand cases and random call sequences, the
configuration checks, the C ABI of dxrl_pg_adam_step_ctl against its ctypes mirror, and the CLI."""
import ctypes as C
import math
import os
import random
import subprocess
import tempfile

import pytest

import pg_lr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dxrl.h")


@pytest.fixture(scope="module")
def native():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        d.build.build_native()
    return _native


def cfg(**kw):
    from dexterous_rl_manipulation_amd.trainer import TrainerConfig
    return TrainerConfig(**kw)


# ------------------------------------------------------------------ schedules
@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_schedule_endpoints_and_monotone(kind):
    from dexterous_rl_manipulation_amd.lr_control import lr_nominal
    for lr, end, n in ((3e-4, 3e-5, 200), (1e-4, 1e-3, 7), (3e-4, 3e-4, 5), (2.5e-4, 1e-6, 1)):
        c = cfg(lr=lr, lr_schedule=kind, lr_final=end, lr_schedule_iterations=n)
        vals = [lr_nominal(c, i) for i in range(n + 4)]
        assert vals[0] == lr and vals[n] == end and all(v == end for v in vals[n:])
        assert vals == [R.schedule(kind, lr, end, n, i) for i in range(n + 4)]  # the restatement, bit for bit
        steps = [b - a for a, b in zip(vals, vals[1:])]
        assert all(d <= 0 for d in steps) if end <= lr else all(d >= 0 for d in steps)
        assert all(min(lr, end) <= v <= max(lr, end) for v in vals)


def test_constant_schedule_is_lr():
    from dexterous_rl_manipulation_amd.lr_control import control_enabled, lr_nominal
    c = cfg(lr=2e-4)
    assert not control_enabled(c) and [lr_nominal(c, i) for i in (0, 1, 10**6)] == [2e-4] * 3
    assert control_enabled(cfg(target_kl=0.01, epochs=2))
    assert control_enabled(cfg(lr_schedule="linear", lr_final=1e-5, lr_schedule_iterations=3))


# ------------------------------------------------------------------ the controller's rules
def run(calls, state=None):
    """calls: (control kwargs, kl_sum, rows) -> the states, decisions and rows of every call."""
    s = state or R.fresh_state()
    out = []
    for kw, kl_sum, rows in calls:
        s, d, row = R.step(s, R.control(**kw), kl_sum, rows)
        out.append((s, d, row))
    return out


def test_stop_rule_by_hand():
    kw = dict(lr_nominal=3e-4, target_kl=0.01, stop_factor=1.5)
    flags = [dict(pass_index=u, last_epoch=int(u >= 2), last_pass=int(u == 3)) for u in range(4)]
    # KL 0, then exactly at 1.5 x target (no stop: strict), then above, then 0 again
    kls = [0.0, 0.015 * 64, 0.016 * 64, 0.0]
    out = run([(dict(kw, **f), k, 64) for f, k in zip(flags, kls)])
    assert [d["applied"] for _, d, _ in out] == [True, True, False, False]  # nothing applied after the stop
    assert [d["t"] for _, d, _ in out] == [1, 2, None, None]
    s, _, row = out[-1]
    assert (s["applied"], s["skipped"], s["stopped"], s["stop_pass"]) == (2, 2, 1, 2)
    assert row == [3e-4, 3e-4, 2.0, 2.0, 2.0, 0.016, (0.016 * 64 + 0.0) / 128.0, 1.0]
    # the next iteration's pass 0 clears the stop and applies with t = applied + 1
    nxt = run([(dict(kw, **flags[0]), 0.0, 64)], state=s)[0]
    assert nxt[1]["applied"] and nxt[1]["t"] == 3 and nxt[0]["stopped"] == 0 and nxt[0]["stop_pass"] == -1
    assert nxt[0]["iter_skipped"] == 0 and nxt[0]["skipped"] == 2


def test_negative_kl_is_below_every_threshold_and_adapts_up():
    kw = dict(lr_nominal=3e-4, target_kl=0.01, adapt=1)
    out = run([(dict(kw, pass_index=0, last_epoch=1, last_pass=1), -5.0, 100)])
    s, d, row = out[0]
    assert d["applied"] and row[6] == -0.05 and s["scale"] == 1.5 and row[7] == 1.5


def test_adaptation_once_per_iteration_and_band():
    kw = dict(lr_nominal=3e-4, target_kl=0.01, adapt=1, stop_factor=math.inf)
    # two passes in the last epoch: kl_epoch = (3 + 1) / 200 = 0.02 -- exactly band x target: no change
    calls = [(dict(kw, pass_index=0, last_epoch=0, last_pass=0), 50.0, 100),
             (dict(kw, pass_index=1, last_epoch=1, last_pass=0), 3.0, 100),
             (dict(kw, pass_index=2, last_epoch=1, last_pass=1), 1.0, 100)]
    out = run(calls)
    assert [s["scale"] for s, _, _ in out] == [1.0, 1.0, 1.0] and out[-1][2][6] == 0.02
    assert all(d["applied"] for _, d, _ in out)  # stop_factor inf: adapt without stopping
    calls[2] = (calls[2][0], 1.0 + 2.0 ** -20, 100)
    out = run(calls)
    assert out[-1][0]["scale"] == 1.0 / 1.5 and out[1][0]["scale"] == 1.0
    # the new scale is the next iteration's learning rate
    nxt = run([(dict(kw, pass_index=0, last_epoch=1, last_pass=1), 1.0, 100)], state=out[-1][0])
    assert nxt[0][1]["lr"] == 3e-4 * (1.0 / 1.5)


def test_random_calls_keep_the_invariants():
    rng = random.Random(1234)
    s = R.fresh_state()
    lr_min, lr_max, target = 1e-5, 2e-3, 0.01
    pass_index, stopped_seen, applied = 0, False, 0
    lr_nominal = 3e-4
    for call in range(10000):
        if pass_index == 0:
            lr_nominal = 10.0 ** rng.uniform(-6.5, -2.0)  # also outside [lr_min, lr_max]
            stopped_seen = False
        last_pass = int(rng.random() < 0.2)
        c = R.control(lr_nominal, lr_min, lr_max, target, rng.choice([1.5, 1.0, math.inf]), adapt=1,
                      adapt_factor=rng.choice([1.5, 2.0, 1.1]), adapt_band=rng.choice([1.0, 2.0]),
                      pass_index=pass_index, last_epoch=int(last_pass or rng.random() < 0.5), last_pass=last_pass)
        rows = rng.choice([32, 1280, 4096])
        kl_sum = rng.choice([-1.0, 0.0, 0.3, 1.0, 1.5, 2.0, 4.0]) * target * rows + rng.randrange(-3, 4) * 2.0 ** -20
        before = dict(s)
        s, d, row = R.step(s, c, kl_sum, rows)
        assert s["applied"] + s["skipped"] == call + 1
        if pass_index == 0:  # the stop clears at pass 0: only this pass's own KL can stop it
            assert d["applied"] == (not d["kl"] > c["stop_factor"] * target)
        if stopped_seen:
            assert not d["applied"]  # no pass is applied after a stop within an iteration
        stopped_seen = stopped_seen or not d["applied"]
        if d["applied"]:
            applied += 1
            assert d["t"] == applied == s["applied"]  # t counts applied passes only
            assert lr_min <= d["lr"] <= lr_max
        else:
            assert s["applied"] == before["applied"] and s["skipped"] == before["skipped"] + 1
        if last_pass:
            assert lr_min <= lr_nominal * s["scale"] <= lr_max
            assert row[2] + row[3] == pass_index + 1 and row[7] == s["scale"]
            assert (row[4] == -1.0) == (row[3] == 0.0)
        else:
            assert s["scale"] == before["scale"] and row is None
        pass_index = 0 if last_pass else pass_index + 1
    assert s["skipped"] > 1000 and s["applied"] > 1000


# ------------------------------------------------------------------ configuration checks
def test_validation_cases():
    from dexterous_rl_manipulation_amd.lr_control import validate_lr_control as v
    v(cfg())  # the defaults
    v(cfg(target_kl=0.01, epochs=2, minibatches=2, kl_adaptive=True))
    v(cfg(lr_schedule="cosine", lr_final=1e-5, lr_schedule_iterations=10))
    v(cfg(lr_schedule="linear", lr_final=1e-5, lr_schedule_iterations=10, fused=False))  # no KL rule: any learner
    v(cfg(target_kl=0.01, minibatches=4))  # stop only: one epoch of several passes is enough
    bad = [dict(target_kl=0.01),                                       # 1 x 1: the only pass sees ratio 1
           dict(target_kl=0.01, kl_adaptive=True, minibatches=4),      # adaptive with one epoch
           dict(kl_adaptive=True, epochs=4),                           # adaptive without a target
           dict(kl_adaptive=True, epochs=4, lr_schedule="linear", lr_final=1e-5, lr_schedule_iterations=3),
           dict(lr_schedule="linear"), dict(lr_schedule="cosine", lr_final=1e-5),
           dict(lr_schedule="cosine", lr_schedule_iterations=5),
           dict(target_kl=0.01, epochs=2, lr_min=1e-2, lr_max=1e-3),   # lr_min > lr_max
           dict(lr_schedule="linear", lr_final=1e-5, lr_schedule_iterations=3, lr_min=1e-2, lr_max=1e-3),
           dict(target_kl=0.01, epochs=2, fused=False),                # a KL rule on the GEMM chain
           dict(lr_schedule="step"), dict(target_kl=-1.0, epochs=2), dict(target_kl=0.0, epochs=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            v(cfg(**kw))
    with pytest.raises(ValueError, match="lr_min"):
        v(cfg(target_kl=0.01, epochs=2, lr_min=1e-2, lr_max=1e-3))
    with pytest.raises(ValueError, match="ratio 1"):
        v(cfg(target_kl=0.01))


# ------------------------------------------------------------------ C ABI
def test_abi_constants_and_struct(native):
    """dxrl_pg_lr_control, the state slots and the row columns against _native.py, by a gcc-compiled probe."""
    slots = [n for n, _ in native.PG_OPT_SLOTS]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("abi %d\\n", DXRL_ABI_VERSION);', 'printf("named %d\\n", (int)DXRL_PG_OPT_NAMED);',
             'printf("slot_words %d\\n", (int)DXRL_PG_OPT_SLOT_WORDS);',
             'printf("state_words %d\\n", (int)DXRL_PG_OPT_STATE_WORDS);',
             'printf("cols %d\\n", (int)DXRL_PG_OPT_COLS);',
             'printf("size %zu\\n", sizeof(dxrl_pg_lr_control));']
    for n in slots:
        lines.append(f'printf("slot.{n} %d\\n", (int)DXRL_PG_OPT_{n.upper()});')
    for n in native.PG_OPT_COLUMNS:
        lines.append(f'printf("col.{n} %d\\n", (int)DXRL_PG_OPT_COL_{n.upper()});')
    for f, _ in native.PgLrControl._fields_:
        lines.append(f'printf("field.{f} %zu\\n", offsetof(dxrl_pg_lr_control, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got["abi"]) == native.ABI_VERSION == 1
    assert int(got["named"]) == native.PG_OPT_NAMED == len(R.SLOTS) <= native.PG_OPT_SLOT_WORDS
    assert int(got["slot_words"]) == native.PG_OPT_SLOT_WORDS == R.SLOT_WORDS
    assert int(got["state_words"]) == native.PG_OPT_STATE_WORDS == 2 * R.SLOT_WORDS
    assert int(got["cols"]) == native.PG_OPT_COLS == len(R.COLUMNS) == 8
    assert tuple(slots) == R.SLOTS and native.PG_OPT_COLUMNS == R.COLUMNS
    assert [n for n, t in native.PG_OPT_SLOTS if t == "i64"] == list(R.INT_SLOTS)
    for k, n in enumerate(slots):
        assert int(got[f"slot.{n}"]) == k
    for k, n in enumerate(native.PG_OPT_COLUMNS):
        assert int(got[f"col.{n}"]) == k
    assert int(got["size"]) == C.sizeof(native.PgLrControl)
    for f, _ in native.PgLrControl._fields_:
        assert int(got[f"field.{f}"]) == getattr(native.PgLrControl, f).offset, f


def test_entry_rejects_bad_arguments_before_a_device(native):
    fake = C.c_void_p(0x1000)
    k = native.PgLrControl(lr_nominal=3e-4, lr_min=1e-6, lr_max=1e-2, stop_factor=1.5, adapt_factor=1.5,
                           adapt_band=2.0, calls=1)

    def call(n=None, ctl=k, state=fake):
        from dexterous_rl_manipulation_amd.trainer import NPARAMS
        a, b = C.c_void_p(0x2000), C.c_void_p(0x3000)
        native.call("dxrl_pg_adam_step_ctl", 0, a, fake, a, a, b, b, b, NPARAMS if n is None else n, 0.9, 0.999, 1e-5,
                    0.5, fake, 4, fake, fake, fake, 4, 128, ctl, state, None, None)

    with pytest.raises(ValueError, match="padded parameter count"):
        call(n=12345)
    with pytest.raises(ValueError):
        call(state=None)
    for field, value in (("calls", 0), ("lr_min", 1.0), ("lr_nominal", 0.0), ("pass_index", -1), ("target_kl", -1.0)):
        bad = native.PgLrControl.from_buffer_copy(k)
        setattr(bad, field, value)
        with pytest.raises(ValueError, match="adam_step_ctl"):
            call(ctl=bad)


# ------------------------------------------------------------------ log / checkpoint / CLI
def test_optimizer_log_json_round_trip():
    from dexterous_rl_manipulation_amd import training_run as T
    import numpy as np
    table = np.zeros((2, T.COLS))
    header = {"rows_written": 2, "best_row": -1, "converged_row": -1, "best_score": -math.inf}
    opt = [[3e-4, 2e-4, 5.0, 1.0, 5.0, 0.02, 0.011, 0.5], [1.5e-4, 1.5e-4, 6.0, 0.0, -1.0, 0.004, 0.003, 0.75]]
    log = T.TrainingLog(table, header, optimizer=opt)
    assert log.optimizer.column("stop_pass").tolist() == [5.0, -1.0] and len(log.optimizer) == 2
    assert log.optimizer["lr_scale"].tolist() == [0.5, 0.75] and set(log.optimizer.columns) == set(T.OPT_COLUMNS)
    with pytest.raises(ValueError):
        log.optimizer.column("nope")
    d = log.to_dict()
    assert d["optimizer_columns"] == list(T.OPT_COLUMNS)
    back = T.TrainingLog.from_dict(d)
    assert back.optimizer.table.tobytes() == log.optimizer.table.tobytes()
    plain = T.TrainingLog(table, header)
    assert plain.optimizer is None and "optimizer" not in plain.to_dict()
    assert T.TrainingLog.from_dict(plain.to_dict()).optimizer is None


def test_checkpoint_config_entry_is_unchanged_without_the_feature():
    import dataclasses
    from dexterous_rl_manipulation_amd import training_run as T
    from dexterous_rl_manipulation_amd.lr_control import CONFIG_DEFAULTS
    from dexterous_rl_manipulation_amd.trainer import TrainerConfig
    plain = T._trainer_config_state(TrainerConfig(lr=1e-4))
    assert not set(plain) & set(CONFIG_DEFAULTS) and plain["lr"] == 1e-4
    assert TrainerConfig(**dict(plain, betas=tuple(plain["betas"]))) == TrainerConfig(lr=1e-4)
    c = TrainerConfig(target_kl=0.02, kl_adaptive=True, epochs=3)
    state = T._trainer_config_state(c)
    assert state["target_kl"] == 0.02 and state["kl_adaptive"] is True and "lr_min" not in state
    assert TrainerConfig(**dict(state, betas=tuple(state["betas"]))) == c
    assert {f.name: f.default for f in dataclasses.fields(TrainerConfig) if f.name in CONFIG_DEFAULTS} == CONFIG_DEFAULTS


def test_cli_flags():
    from dexterous_rl_manipulation_amd import train
    a = train.parse_args(["--iterations", "3", "--out", "o"])
    assert a.lr_control == {}
    a = train.parse_args(["--iterations", "40", "--out", "o", "--epochs", "4", "--minibatches", "4", "--lr-schedule",
                          "cosine", "--lr-final", "3e-5", "--target-kl", "0.02", "--kl-adaptive", "--lr-min", "1e-5",
                          "--lr-max", "1e-3"])
    assert a.lr_control == dict(lr_schedule="cosine", lr_final=3e-5, lr_schedule_iterations=40, target_kl=0.02,
                                kl_adaptive=True, kl_stop=True, lr_min=1e-5, lr_max=1e-3)
    a = train.parse_args(["--iterations", "4", "--out", "o", "--epochs", "2", "--target-kl", "0.02", "--no-kl-stop"])
    assert a.lr_control == dict(target_kl=0.02, kl_adaptive=False, kl_stop=False)
    for argv in (["--lr-schedule", "linear"], ["--lr-final", "1e-5"], ["--kl-adaptive"], ["--no-kl-stop"],
                 ["--lr-min", "1e-5"], ["--target-kl", "0.02"], ["--target-kl", "0.02", "--epochs", "4", "--gpus", "2"],
                 ["--target-kl", "0.02", "--kl-adaptive", "--minibatches", "4"]):
        with pytest.raises(SystemExit):
            train.parse_args(["--iterations", "3", "--out", "o"] + argv)
