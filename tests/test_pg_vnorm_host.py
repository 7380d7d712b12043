"""CPU checks of value normalisation: the restatement (tests/pg_vnorm_reference.py) that the GPU
tests hold dxrl_pg_gae_vnorm to, the ctypes mirror of its args struct, the configuration checks and
the checkpoint rule."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest
import torch

import pg_reference as R
import pg_timelimit_reference as TL
import pg_vnorm_reference as VN

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dxrl.h")
SCANS = [True, False]  # k_gae_lds's segmented scan, k_gae's sequential chain


def _inputs(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    rew = torch.randn(T * n, generator=g)
    V = torch.randn((T + 1) * n, generator=g) * 50.0
    ends = torch.rand(T * n, generator=g) < 0.1
    lengths = torch.randint(1, 200, (T * n,), generator=g)
    kind = torch.randint(0, 2, (T * n,), generator=g)
    return rew, V, ends, torch.where(ends, (lengths << 1) | kind, torch.zeros_like(lengths))


def no_negative_zero(x):
    return not ((x == 0) & torch.signbit(x)).any()


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("n,T", [(5, 1), (3, 9), (17, 136), (4, 200)])
def test_fresh_state_is_the_plain_gae(n, T, scan):
    """Under mu = 0, sigma = 1: 1 * V + 0 = V and (ret - 0) / 1 = ret, so adv / ret are
    pg_reference.gae's (and the time-limit restatement's) and ret_norm == ret, bit for bit --
    on a V without a -0.0, which decodes to +0.0."""
    rew, V, ends, code = _inputs(n, T, 13 * n + T)
    assert no_negative_zero(V)
    st = VN.fresh_state()
    adv, ret, retn, v = VN.gae_vnorm(rew, ends.to(torch.uint8), V, n, T, 0.99, 0.95, st["mu"], st["sigma"], scan=scan)
    a_ref, r_ref = R.gae(rew, ends.to(torch.uint8), V, n, T, 0.99, 0.95, scan=scan)
    assert torch.equal(adv, a_ref) and torch.equal(ret, r_ref) and torch.equal(retn, ret) and torch.equal(v, V)
    adv, ret, retn, v = VN.gae_vnorm(rew, code, V, n, T, 0.99, 0.95, 0.0, 1.0, timelimit=True, scan=scan)
    a_ref, r_ref = TL.gae_timelimit(rew, code, V, n, T, 0.99, 0.95, scan=scan)
    assert torch.equal(adv, a_ref) and torch.equal(ret, r_ref) and torch.equal(retn, ret) and torch.equal(v, V)


def test_prepared_state_decodes_and_encodes_with_one_pair():
    """By hand, dyadic numbers: mu = 2, sigma = 4, one env, T = 2, gamma = lambda = 0.5.
    vn = (1, 0.5 | 0.25) -> v = (6, 4 | 3); r = (1, 2), no end:
      t = 1: delta = 2 + 0.5 * 3 - 4 = -0.5; A = -0.5; ret = 3.5; retn = (3.5 - 2) / 4 = 0.375
      t = 0: delta = 1 + 0.5 * 4 - 6 = -3; A = -3 + 0.25 * -0.5 = -3.125; ret = 2.875; retn = 0.21875"""
    for scan in SCANS:
        adv, ret, retn, v = VN.gae_vnorm(torch.tensor([1.0, 2.0]), torch.zeros(2, dtype=torch.uint8),
                                         torch.tensor([1.0, 0.5, 0.25]), 1, 2, 0.5, 0.5, 2.0, 4.0, scan=scan)
        assert v.tolist() == [6.0, 4.0, 3.0] and adv.tolist() == [-3.125, -0.5]
        assert ret.tolist() == [2.875, 3.5] and retn.tolist() == [0.21875, 0.375]


@pytest.mark.parametrize("k,size,mean,std", [(1, 1, 3.0, 1.0), (4, 1000, 35.0, 11.0), (7, 333, -2.0e4, 0.5)])
def test_folding_batches_is_the_moments_of_their_concatenation(k, size, mean, std):
    """k folds of two-pass batch triples against the two-pass triple of the concatenation, to the
    1e-9 relative that test_gae_lds_scan_matches_sequential_reference holds the advantage moments
    to (the same merge); mu / sigma are the f32 roundings of the running mean and
    sqrt(M2 / count + eps)."""
    g = torch.Generator().manual_seed(k * size)
    batches = [(torch.randn(size + 17 * i, generator=g) * std + mean).float() for i in range(k)]
    eps = 1e-5
    st = VN.fresh_state()
    for b in batches:
        st = VN.fold(st, VN.batch_triple(b), eps)
    n, m, m2 = VN.batch_triple(torch.cat(batches))
    assert st["calls"] == k and st["running"][0] == n
    assert math.isclose(st["running"][1], m, rel_tol=1e-9, abs_tol=1e-12)
    assert math.isclose(st["running"][2], m2, rel_tol=1e-9, abs_tol=1e-12)
    mu, sigma = torch.tensor(st["running"][1]).float().item(), st["sigma"]
    assert st["mu"] == mu
    assert sigma == torch.tensor(math.sqrt(st["running"][2] / n + eps), dtype=torch.float64).float().item()
    # an empty batch leaves the moments and the constants alone and counts as a call
    again = VN.fold(st, (0.0, 0.0, 0.0), eps)
    assert again["running"] == st["running"] and (again["mu"], again["sigma"]) == (st["mu"], st["sigma"])
    assert again["calls"] == k + 1


def test_args_struct_and_block_words_match_c():
    """dxrl_pg_gae_vnorm_args against its ctypes mirror (size and every offset) and enum
    dxrl_pg_vnorm_word against _native.PG_VNORM, by a gcc-compiled probe over include/dxrl.h."""
    from dexterous_rl_manipulation_amd import _native as N
    s, mirror = "dxrl_pg_gae_vnorm_args", N.PgGaeVnormArgs
    assert dict(N.LATER_STRUCTS)[s] is mirror
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));', 'printf("words %d\\n", (int)DXRL_PG_VNORM_WORDS);',
             'printf("named %d\\n", (int)DXRL_PG_VNORM_NAMED);', 'printf("abi %d\\n", DXRL_ABI_VERSION);']
    for f, _ in mirror._fields_:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    for w in N.PG_VNORM_NAMES:
        lines.append(f'printf("word.{w} %d\\n", (int)DXRL_PG_VNORM_{w.upper()});')
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
    assert int(got["words"]) == N.PG_VNORM_WORDS and int(got["named"]) == N.PG_VNORM_NAMED <= N.PG_VNORM_WORDS
    assert int(got["abi"]) == N.ABI_VERSION
    for w in N.PG_VNORM_NAMES:
        assert int(got[f"word.{w}"]) == N.PG_VNORM[w], w
    # the six doubles ranks exchange are contiguous: the return triple, then the advantage triple
    assert [N.PG_VNORM[w] for w in ("batch_count", "batch_mean", "batch_m2", "adv_count", "adv_mean", "adv_m2")] \
        == list(range(N.PG_VNORM["batch_count"], N.PG_VNORM["batch_count"] + 6))
    fresh = N.vnorm_fresh()
    assert fresh.dtype == torch.float64 and fresh.numel() == N.PG_VNORM_WORDS
    assert fresh[N.PG_VNORM["sigma"]] == 1.0 and fresh.sum() == 1.0


def test_config_validation_cli_flags_and_checkpoint_rule():
    """TrainerConfig.value_norm defaults to False; a negative or non-finite value_norm_eps is
    refused; train --value-norm [--value-norm-eps E] sets the fields (refused on a --resume run);
    the checkpoint's trainer_config carries the fields only when set, an entry without them loads as
    the default, and a file whose block and field disagree raises naming value_norm."""
    from types import SimpleNamespace

    from dexterous_rl_manipulation_amd import train, value_norm
    from dexterous_rl_manipulation_amd import training_run as T
    from dexterous_rl_manipulation_amd.trainer import TrainerConfig
    assert TrainerConfig().value_norm is False and TrainerConfig().value_norm_eps == 1e-5
    value_norm.validate_value_norm(TrainerConfig())
    value_norm.validate_value_norm(TrainerConfig(value_norm=True, value_norm_eps=0.0))
    for bad in (-1e-9, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="value_norm_eps"):
            value_norm.validate_value_norm(SimpleNamespace(value_norm=True, value_norm_eps=bad))
    base = ["--iterations", "1", "--out", "x"]
    a = train.parse_args(base)
    assert a.value_norm is False and a.value_norm_eps is None
    a = train.parse_args(base + ["--value-norm", "--value-norm-eps", "1e-3"])
    assert a.value_norm is True and a.value_norm_eps == 1e-3
    for bad in (["--value-norm", "--resume", "ck.npz"], ["--value-norm-eps", "1e-3"],
                ["--value-norm", "--value-norm-eps", "-1"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)
    plain = T._trainer_config_state(TrainerConfig())
    assert "value_norm" not in plain and "value_norm_eps" not in plain
    state = T._trainer_config_state(TrainerConfig(value_norm=True))
    assert state["value_norm"] is True and "value_norm_eps" not in state
    state["betas"] = tuple(state["betas"])
    assert TrainerConfig(**state) == TrainerConfig(value_norm=True)
    state.pop("value_norm")
    assert TrainerConfig(**state) == TrainerConfig()
    assert T._trainer_config_state(TrainerConfig(value_norm=True, value_norm_eps=1e-3))["value_norm_eps"] == 1e-3
    value_norm.check_checkpoint(False, False)
    value_norm.check_checkpoint(True, True)
    for cfg_on, has_block in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="value_norm"):
            value_norm.check_checkpoint(cfg_on, has_block, "ck.npz")


def test_state_dict_names_the_block():
    from dexterous_rl_manipulation_amd import _native as N
    from dexterous_rl_manipulation_amd import value_norm
    block = [0.0] * N.PG_VNORM_WORDS
    for name, v in (("count", 4.0), ("mean", 2.0), ("m2", 36.0), ("mu", 2.0), ("sigma", 3.0), ("batch_count", 2.0),
                    ("batch_mean", 1.0), ("batch_m2", 8.0), ("calls", 3.0)):
        block[N.PG_VNORM[name]] = v
    assert value_norm.state_dict(block) == {"count": 4.0, "mean": 2.0, "std": 3.0, "mu": 2.0, "sigma": 3.0,
                                            "batch_mean": 1.0, "batch_std": 2.0, "calls": 3}
    assert value_norm.state_dict(N.vnorm_fresh().tolist())["std"] == 0.0


def test_studies_forward_the_fields_to_trainer_config(monkeypatch):
    """training_study.run_training_study hands its extra keywords to make_job untouched, and
    reward_comparison.run_training_comparison builds its TrainerConfig from them: neither filters
    value_norm / value_norm_eps out.  The device-facing constructors are replaced by recorders that
    stop the run."""
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
                                          value_norm=True, value_norm_eps=1e-3)
    assert seen["job"]["value_norm"] is True and seen["job"]["value_norm_eps"] == 1e-3

    def trainer_stub(env, cfg, **kw):
        seen["cfg"] = cfg
        raise Stop

    monkeypatch.setattr(envs, "VecEnv", lambda *a, **kw: object())
    monkeypatch.setattr(trainer, "PGTrainer", trainer_stub)
    with pytest.raises(Stop):
        reward_comparison.run_training_comparison("dense", 1, value_norm=True, value_norm_eps=1e-3)
    assert seen["cfg"].value_norm is True and seen["cfg"].value_norm_eps == 1e-3
    with pytest.raises(Stop):
        reward_comparison.compare_rewards(1, value_norm=True)
    assert seen["cfg"].value_norm is True
