"""CPU checks of PopArt and the forgetting fold: the restatement (tests/pg_popart_reference.py) that
the GPU tests hold dxrl_pg_popart_rescale and the fold to, the ctypes mirrors against include/dxrl.h,
the configuration checks, the CLI flags and the checkpoint rules."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import pg_popart_reference as PA
import pg_vnorm_reference as VN

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dxrl.h")


def test_rescale_by_hand_preserves_the_decoded_value_exactly():
    """Dyadic numbers, every product and quotient exact: (mu_h, sigma_h) = (2, 4) -> (mu_n, sigma_n)
    = (-6, 8).  s = 4 / 8 = 0.5; w = (1, -0.5, 0.25, 0, -0, ...) -> w' = (0.5, -0.25, 0.125, 0, -0,
    ...); b = 1.5 -> b' = (4 * 1.5 + (2 - -6)) / 8 = 14 / 8 = 1.75; shift = 8 / 8 = 1.
    With h = (1, 1, -1, ...): w h + b = 1 - 0.5 - 0.25 + 1.5 = 1.75, decoded 4 * 1.75 + 2 = 9;
    w' h + b' = 0.5 - 0.25 - 0.125 + 1.75 = 1.875, decoded 8 * 1.875 - 6 = 9."""
    head = np.zeros(PA.HEAD, dtype=np.float32)
    head[:5] = [1.0, -0.5, 0.25, 0.0, -0.0]
    head[256] = 1.5
    new, s, shift = PA.rescale_head(head, 2.0, 4.0, -6.0, 8.0)
    assert (s, shift) == (0.5, 1.0)
    assert new[:5].tolist() == [0.5, -0.25, 0.125, 0.0, 0.0] and np.signbit(new[4]) and not np.signbit(new[3])
    assert new[256] == 1.75 and not new[5:256].any()
    h = np.zeros((1, 256))
    h[0, :3] = [1.0, 1.0, -1.0]
    assert PA.decoded(head, h, 2.0, 4.0)[0] == 9.0
    assert PA.decoded(new, h, -6.0, 8.0)[0] == PA.decoded(head, h, 2.0, 4.0)[0]
    # the call: the block moves to the new pair, the row names both
    vn = dict.fromkeys(("count", "mean", "m2", "batch_count", "batch_mean", "batch_m2", "calls", "forget"), 0.0)
    vn.update(mu=-6.0, sigma=8.0, count=4.0, m2=36.0, calls=2.0)
    block = dict(PA.fresh_block(), mu_head=2.0, sigma_head=4.0)
    got, after, row = PA.popart_call(head, block, vn)
    assert got.tobytes() == new.tobytes()
    assert after == {"mu_head": -6.0, "sigma_head": 8.0, "rescales": 1.0, "skipped": 0.0, "last_scale": 0.5,
                     "last_shift": 1.0}
    assert (row["mu"], row["sigma"], row["mu_prev"], row["sigma_prev"], row["rescaled"], row["std"]) == \
        (-6.0, 8.0, 2.0, 4.0, 1.0, 3.0)
    # the same call again: a no-op with a row; a refused pair: nothing but the counter
    again, same, row = PA.popart_call(got, after, vn)
    assert again.tobytes() == got.tobytes() and same == after
    assert (row["rescaled"], row["scale"], row["shift"]) == (0.0, 1.0, 0.0)
    for bad in (dict(sigma=0.0), dict(sigma=math.inf), dict(mu=math.nan), dict(sigma=-1.0)):
        kept, counted, row = PA.popart_call(got, after, dict(vn, **bad))
        assert row is None and kept.tobytes() == got.tobytes() and counted == dict(after, skipped=1.0)
    assert PA.case(0.0, 1.0, 0.0, 1.0) == "noop" and PA.case(-0.0, 1.0, 0.0, 1.0) == "rescale"  # bitwise


@pytest.mark.parametrize("k,size,mean,std", [(1, 1, 3.0, 1.0), (4, 1000, 35.0, 11.0), (7, 333, -2.0e4, 0.5)])
def test_fold_forget_zero_is_the_plain_fold(k, size, mean, std):
    g = torch.Generator().manual_seed(k * size)
    a, b = VN.fresh_state(), VN.fresh_state()
    for i in range(k):
        t = VN.batch_triple((torch.randn(size + 17 * i, generator=g) * std + mean).float())
        a, b = VN.fold(a, t, 1e-5), PA.fold_forget(b, t, 1e-5, 0.0)
        assert a == b


@pytest.mark.parametrize("forget", [0.01, 0.25, 0.9])
@pytest.mark.parametrize("k,size,mean,std", [(1, 1, 3.0, 1.0), (4, 1000, 35.0, 11.0), (7, 333, -2.0e4, 0.5)])
def test_fold_forget_is_the_weighted_moments(k, size, mean, std, forget):
    """k folds against the explicitly weighted two-pass moments (batch i of k weighs
    (1 - forget) ** (k - 1 - i)), to the 1e-9 relative that the plain fold's test holds its triples
    to; (mu, sigma) are the f32 roundings of the running mean and sqrt(M2 / count + eps)."""
    g = torch.Generator().manual_seed(k * size)
    batches = [(torch.randn(size + 17 * i, generator=g) * std + mean).float() for i in range(k)]
    st = VN.fresh_state()
    for b in batches:
        st = PA.fold_forget(st, VN.batch_triple(b), 1e-5, forget)
    n, m, m2 = PA.weighted_moments([b.numpy() for b in batches], forget)
    assert st["calls"] == k
    assert math.isclose(st["running"][0], n, rel_tol=1e-9)
    assert math.isclose(st["running"][1], m, rel_tol=1e-9, abs_tol=1e-12)
    assert math.isclose(st["running"][2], m2, rel_tol=1e-9, abs_tol=1e-12)
    assert (st["mu"], st["sigma"]) == VN.constants(st["running"], 1e-5)


def test_effective_count_settles_near_a_batch_over_forget():
    st = VN.fresh_state()
    for _ in range(400):
        st = PA.fold_forget(st, (1000.0, 1.0, 500.0), 1e-5, 0.05)
    assert math.isclose(st["running"][0], 1000.0 / 0.05, rel_tol=1e-6)


def test_struct_enums_and_grown_vnorm_words_match_c():
    """dxrl_pg_popart_args against its ctypes mirror, enum dxrl_pg_popart_word and enum
    dxrl_pg_vnorm_log_col against _native's names, and the grown enum dxrl_pg_vnorm_word, by a
    gcc-compiled probe over include/dxrl.h."""
    from dexterous_rl_manipulation_amd import _native as N
    s, mirror = "dxrl_pg_popart_args", N.PgPopartArgs
    assert dict(N.LATER_STRUCTS)[s] is mirror
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));', 'printf("pwords %d\\n", (int)DXRL_PG_POPART_WORDS);',
             'printf("pnamed %d\\n", (int)DXRL_PG_POPART_NAMED);', 'printf("cols %d\\n", (int)DXRL_PG_VNORM_LOG_COLS);',
             'printf("vnamed %d\\n", (int)DXRL_PG_VNORM_NAMED);', 'printf("vwords %d\\n", (int)DXRL_PG_VNORM_WORDS);']
    for f, _ in mirror._fields_:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    for w in N.PG_POPART_NAMES:
        lines.append(f'printf("pword.{w} %d\\n", (int)DXRL_PG_POPART_{w.upper()});')
    for w in N.PG_VNORM_LOG_COLUMNS:
        lines.append(f'printf("col.{w} %d\\n", (int)DXRL_PG_VNORM_LOG_{w.upper()});')
    for w in N.PG_VNORM_NAMES:
        lines.append(f'printf("vword.{w} %d\\n", (int)DXRL_PG_VNORM_{w.upper()});')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got[s]) == C.sizeof(mirror)
    for f, _ in mirror._fields_:
        assert int(got[f"{s}.{f}"]) == getattr(mirror, f).offset, f
    assert int(got["pwords"]) == N.PG_POPART_WORDS == 8 and int(got["pnamed"]) == N.PG_POPART_NAMED <= N.PG_POPART_WORDS
    assert int(got["cols"]) == N.PG_VNORM_LOG_COLS == len(N.PG_VNORM_LOG_COLUMNS)
    for w in N.PG_POPART_NAMES:
        assert int(got[f"pword.{w}"]) == N.PG_POPART[w], w
    for k, w in enumerate(N.PG_VNORM_LOG_COLUMNS):
        assert int(got[f"col.{w}"]) == k, w
    for w in N.PG_VNORM_NAMES:
        assert int(got[f"vword.{w}"]) == N.PG_VNORM[w], w
    # FORGET took the first spare word; the block did not grow
    assert N.PG_VNORM_NAMES[-1] == "forget" and N.PG_VNORM["forget"] == N.PG_VNORM["eps"] + 1 == 13
    assert int(got["vnamed"]) == N.PG_VNORM_NAMED == 14 and int(got["vwords"]) == N.PG_VNORM_WORDS == 16
    fresh = N.popart_fresh()
    assert fresh.dtype == torch.float64 and fresh.numel() == N.PG_POPART_WORDS
    assert fresh[N.PG_POPART["sigma_head"]] == 1.0 and fresh.sum() == 1.0
    assert N.vnorm_fresh()[N.PG_VNORM["forget"]] == 0.0 and N.vnorm_fresh().sum() == 1.0


def test_config_validation_cli_flags_and_checkpoint_rules():
    from types import SimpleNamespace

    from dexterous_rl_manipulation_amd import _native as N
    from dexterous_rl_manipulation_amd import train, value_norm
    from dexterous_rl_manipulation_amd import training_run as T
    from dexterous_rl_manipulation_amd.trainer import TrainerConfig
    assert TrainerConfig().popart is False and TrainerConfig().value_norm_forget == 0.0
    value_norm.validate_value_norm(TrainerConfig())
    value_norm.validate_value_norm(TrainerConfig(value_norm=True, popart=True, value_norm_forget=0.05))
    value_norm.validate_value_norm(TrainerConfig(value_norm=True, value_norm_forget=0.0))
    with pytest.raises(ValueError, match="popart"):
        value_norm.validate_value_norm(TrainerConfig(popart=True))
    with pytest.raises(ValueError, match="value_norm_forget"):
        value_norm.validate_value_norm(TrainerConfig(value_norm_forget=0.1))
    for bad in (-1e-9, 1.0, 1.5, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="value_norm_forget"):
            value_norm.validate_value_norm(SimpleNamespace(value_norm=True, value_norm_eps=1e-5, popart=False,
                                                           value_norm_forget=bad))
    # the CLI
    base = ["--iterations", "1", "--out", "x"]
    a = train.parse_args(base)
    assert a.popart is False and a.value_norm_forget is None
    a = train.parse_args(base + ["--value-norm", "--popart", "--value-norm-forget", "0.02"])
    assert a.value_norm and a.popart is True and a.value_norm_forget == 0.02
    assert train.parse_args(base + ["--value-norm", "--popart"]).value_norm_forget is None
    for bad in (["--popart"], ["--value-norm-forget", "0.1"], ["--value-norm", "--value-norm-forget", "1.0"],
                ["--value-norm", "--value-norm-forget", "-0.1"], ["--value-norm", "--popart", "--resume", "ck.npz"],
                ["--popart", "--resume", "ck.npz"], ["--value-norm-forget", "0.1", "--resume", "ck.npz"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)
    # the checkpoint's trainer_config carries the fields only when set; a missing field loads as the default
    plain = T._trainer_config_state(TrainerConfig(value_norm=True))
    assert "popart" not in plain and "value_norm_forget" not in plain
    state = T._trainer_config_state(TrainerConfig(value_norm=True, popart=True, value_norm_forget=0.05))
    assert state["popart"] is True and state["value_norm_forget"] == 0.05
    state["betas"] = tuple(state["betas"])
    assert TrainerConfig(**state) == TrainerConfig(value_norm=True, popart=True, value_norm_forget=0.05)
    state.pop("popart"), state.pop("value_norm_forget")
    assert TrainerConfig(**state) == TrainerConfig(value_norm=True)
    # a file whose block and field disagree raises naming popart
    value_norm.check_popart_checkpoint(False, False)
    value_norm.check_popart_checkpoint(True, True)
    for cfg_on, has_block in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="popart"):
            value_norm.check_popart_checkpoint(cfg_on, has_block, "ck.npz")
    # a vnorm block whose FORGET word disagrees with the configuration raises naming value_norm_forget
    block = N.vnorm_fresh().numpy()
    value_norm.check_forget(0.0, block)
    with pytest.raises(ValueError, match="value_norm_forget"):
        value_norm.check_forget(0.05, block, "ck.npz")
    block[N.PG_VNORM["forget"]] = 0.05
    value_norm.check_forget(0.05, block)
    with pytest.raises(ValueError, match="value_norm_forget"):
        value_norm.check_forget(0.0, block, "ck.npz")
    assert value_norm.popart_dict(N.popart_fresh().tolist()) == {
        "mu_head": 0.0, "sigma_head": 1.0, "rescales": 0, "skipped": 0, "last_scale": 0.0, "last_shift": 0.0}
    # value_norm_state() keeps its keys
    assert "forget" not in value_norm.state_dict(N.vnorm_fresh().tolist())


def test_value_norm_log_rides_the_json():
    from dexterous_rl_manipulation_amd import training_run as T
    table = np.zeros((2, T.COLS))
    header = {"rows_written": 2, "best_row": -1, "converged_row": -1, "best_score": -math.inf}
    rows = np.arange(2 * T.VNORM_COLS, dtype=np.float64).reshape(2, T.VNORM_COLS)
    v = T.ValueNormLog(rows)
    assert len(v) == 2 and v["sigma"].tolist() == [1.0, 1.0 + T.VNORM_COLS] and set(v.columns) == set(T.VNORM_COLUMNS)
    with pytest.raises(ValueError, match="value_norm column"):
        v.column("nope")
    log = T.TrainingLog(table, header, value_norm=rows)
    assert log.to_dict()["value_norm_columns"] == list(T.VNORM_COLUMNS)
    back = T.TrainingLog.from_dict(log.to_dict())
    assert np.array_equal(back.value_norm.table, rows)
    plain = T.TrainingLog(table, header)
    assert plain.value_norm is None and "value_norm" not in plain.to_dict()
    assert T.TrainingLog.from_dict(plain.to_dict()).value_norm is None


def test_studies_forward_the_fields_to_trainer_config(monkeypatch):
    """As for value_norm: neither training_study.run_training_study nor
    reward_comparison.run_training_comparison filters popart / value_norm_forget out."""
    from dexterous_rl_manipulation_amd import envs, reward_comparison, trainer, training_study

    class Stop(Exception):
        pass

    seen = {}

    def make_job(arm, seed, **kw):
        seen["job"] = kw
        raise Stop

    monkeypatch.setattr(training_study.N, "require_gpu", lambda device: torch.device("cpu"))
    monkeypatch.setattr(training_study, "make_job", make_job)
    with pytest.raises(Stop):
        training_study.run_training_study([training_study.Arm("fixed", False, "dense")], [42], 1, validate_every=0,
                                          value_norm=True, popart=True, value_norm_forget=0.05)
    assert seen["job"]["popart"] is True and seen["job"]["value_norm_forget"] == 0.05

    def trainer_stub(env, cfg, **kw):
        seen["cfg"] = cfg
        raise Stop

    monkeypatch.setattr(envs, "VecEnv", lambda *a, **kw: object())
    monkeypatch.setattr(trainer, "PGTrainer", trainer_stub)
    with pytest.raises(Stop):
        reward_comparison.run_training_comparison("dense", 1, value_norm=True, popart=True, value_norm_forget=0.05)
    assert seen["cfg"].popart is True and seen["cfg"].value_norm_forget == 0.05
