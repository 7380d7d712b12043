"""CPU checks of the MLP-actor evaluation surface: policies.MLPActorPolicy (host forward, streams,
save / load), its policy program, and the C ABI of dxrl_evaluate_mlp (struct layout, argument
checks that run before any device is touched)."""
import copy
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import eval_mlp_reference as E
import pg_reference as R
from test_eval_host import make_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dxrl.h")


@pytest.fixture(scope="module")
def native():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        d.build.build_native()
    return _native


def observations(n=64, seed=3):
    rng = np.random.default_rng(seed)
    obs = np.zeros((n, 45), np.float32)
    obs[:, :15] = rng.uniform(-0.6, 0.6, (n, 15))
    obs[:, 15:30] = rng.uniform(-0.3, 0.3, (n, 15))
    obs[:, 30:33] = rng.uniform(-0.2, 0.3, (n, 3))
    obs[:, 33] = 1.0
    obs[:, 37:40] = rng.uniform(-0.1, 0.1, (n, 3))
    obs[:, 40:45] = rng.integers(0, 2, (n, 5))
    return obs


@pytest.mark.parametrize("deterministic", [True, False])
def test_select_action_matches_restatement(deterministic):
    params = E.actor_params(0)
    pol = E.policy_of(params, deterministic=deterministic, seed=11)
    obs = observations()
    mu = E.mu_ref(obs, params, bf16=True).numpy()
    want = mu
    if not deterministic:
        g = copy.deepcopy(pol.rng).standard_normal((len(obs), 15))  # the draws select_action will take
        std = torch.exp(R.unpack(params)["logstd"]).numpy()
        want = mu + (0.0 + std.astype(np.float64) * g).astype(np.float32)
    want = np.clip(want, -1.0, 1.0)
    clipped, inside = E.clip_shares(want)
    assert clipped >= 0.02 and inside >= 0.5, (clipped, inside)
    got = np.stack([pol.select_action(o) for o in obs])
    assert got.dtype == np.float32 and got.shape == (len(obs), 15)
    assert np.abs(got - want).max() <= 1e-6
    pol.reset()
    assert pol.action_space.shape == (15,) and np.all(pol.action_space.low == -1) and np.all(pol.action_space.high == 1)


def test_save_load_round_trip_is_bitwise(tmp_path):
    params = E.actor_params(4)
    pol = E.policy_of(params, deterministic=False, seed=2)
    path = tmp_path / "actor.npz"
    pol.save(path)
    from dexterous_rl_manipulation_amd.policies import MLPActorPolicy
    back = MLPActorPolicy.load(path)
    for k in ("W1a", "W2a", "W3a", "logstd", "std"):
        assert torch.equal(getattr(pol, k), getattr(back, k)), k
    assert back.deterministic is False
    W = R.unpack(params)
    assert torch.equal(back.W1a, W["W1a"]) and torch.equal(back.W2a, W["W2a"]) and torch.equal(back.W3a, W["W3a"])
    assert torch.equal(back.logstd, W["logstd"])
    obs = observations(4)
    det = E.policy_of(params)
    det.save(path)
    assert MLPActorPolicy.load(path).deterministic is True
    assert np.array_equal(MLPActorPolicy.load(path).select_action(obs[0]), det.select_action(obs[0]))
    np.savez(open(path, "wb"), format=np.array("something-else"))
    with pytest.raises(ValueError):
        MLPActorPolicy.load(path)


def test_snapshot_is_a_private_copy():
    params = E.actor_params(1)
    pol = E.policy_of(params)
    before = pol.select_action(observations(1)[0])
    params.mul_(0.5)
    assert np.array_equal(pol.select_action(observations(1)[0]), before)


def test_policy_stream_peek_and_commit():
    from dexterous_rl_manipulation_amd import evaluator as evr
    pol = E.policy_of(E.actor_params(0), deterministic=False, seed=5)
    prog = evr.policy_program(pol)
    want = evr._pcg(5).standard_normal(100)
    assert np.array_equal(prog.stream.draw(40), want[:40])
    assert np.array_equal(prog.stream.draw(40), want[:40])  # peeking does not advance
    prog.stream.commit(30)
    assert np.array_equal(prog.stream.draw(20), want[30:50])
    prog.stream.commit(0)
    assert np.array_equal(pol.rng.standard_normal(5), want[30:35])  # the policy's own generator moved by 30
    assert np.array_equal(prog.seeded(9, 7), evr._pcg(9).standard_normal(7))
    assert np.array_equal(pol.seeded(9, 7), evr._pcg(9).standard_normal(7))


def test_policy_program_kinds(native):
    from dexterous_rl_manipulation_amd import evaluator as evr
    det = evr.policy_program(E.policy_of(E.actor_params(0)))
    sto = evr.policy_program(E.policy_of(E.actor_params(0), deterministic=False, seed=1))
    assert det.kind == sto.kind == native.EVAL_POLICY_MLP == 3
    assert det.draws == 0 and sto.draws == 15 and det.mlp is not None
    mean = np.linspace(-0.4, 0.4, 15).astype(np.float32)
    for name, kind in (("simple", native.EVAL_POLICY_SIMPLE), ("heuristic", native.EVAL_POLICY_HEURISTIC),
                       ("random", native.EVAL_POLICY_RANDOM)):
        prog = evr.policy_program(make_policy(name, mean, 3))
        assert prog.kind == kind and prog.mlp is None and prog.draws == 15
    assert (native.EVAL_POLICY_SIMPLE, native.EVAL_POLICY_HEURISTIC, native.EVAL_POLICY_RANDOM) == (0, 1, 2)

    class Other:
        def select_action(self, obs):
            return np.zeros(15, np.float32)

    with pytest.raises(TypeError):
        evr.policy_program(Other())
    assert evr.compiled_program(Other()) is None


def test_eval_mlp_struct_layout_matches_c(native):
    """dxrl_eval_mlp against its ctypes mirror, by a gcc-compiled probe (as test_native_abi does)."""
    s, mirror = "dxrl_eval_mlp", native.EvalMlp
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));', 'printf("policy %d\\n", DXRL_EVAL_POLICY_MLP);',
             'printf("abi %d\\n", DXRL_ABI_VERSION);']
    for f, _ in mirror._fields_:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
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
    assert int(got["policy"]) == native.EVAL_POLICY_MLP and int(got["abi"]) == native.ABI_VERSION == 1


def test_entry_rejects_null_arguments_and_evaluate_rejects_policy_3(native):
    a, m = native.EvalArgs(), native.EvalMlp()
    a.policy = native.EVAL_POLICY_MLP
    with pytest.raises(ValueError, match="null env / args / mlp"):
        native.call("dxrl_evaluate_mlp", None, C.byref(a), C.byref(m), None)
    with pytest.raises(ValueError, match="null env / args"):
        native.call("dxrl_evaluate", None, C.byref(a), None)
    # dxrl_evaluate still refuses the MLP policy (a handle is needed to get that far: a zeroed
    # stand-in, never dereferenced past the checks, is enough -- the policy check comes second)
    fake = (C.c_char * 4096)()
    a.num_lanes = 0
    with pytest.raises(ValueError, match="num_lanes"):
        native.call("dxrl_evaluate", C.addressof(fake), C.byref(a), None)
    fake_cfg = native.EnvConfig.from_buffer(fake)
    fake_cfg.num_envs = 4
    a.num_lanes = 1
    with pytest.raises(ValueError, match="unknown policy 3"):
        native.call("dxrl_evaluate", C.addressof(fake), C.byref(a), None)
    a.policy = native.EVAL_POLICY_SIMPLE
    with pytest.raises(ValueError, match="DXRL_EVAL_POLICY_MLP"):
        native.call("dxrl_evaluate_mlp", C.addressof(fake), C.byref(a), C.byref(m), None)
