"""CPU checks of the time-limit restatement (tests/pg_timelimit_reference.py) that the GPU tests
hold dxrl_pg_gae_timelimit to: its two degenerate tapes against pg_reference.gae, a hand-worked
example, and the property the feature exists for."""
import pytest
import torch

import pg_reference as R
import pg_timelimit_reference as TL

SCANS = [True, False]  # k_gae_lds's segmented scan, k_gae's sequential chain


def _inputs(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    rew = torch.randn(T * n, generator=g)
    V = torch.randn((T + 1) * n, generator=g) * 50.0
    ends = torch.rand(T * n, generator=g) < 0.1
    lengths = torch.randint(1, 200, (T * n,), generator=g)
    return rew, V, ends, lengths


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("n,T", [(5, 1), (3, 9), (17, 136), (4, 200)])
def test_terminations_only_is_plain_gae(n, T, scan):
    """Every code has bit 0 set: the bytes of pg_reference.gae with done = code != 0."""
    rew, V, ends, lengths = _inputs(n, T, 7 * n + T)
    code = torch.where(ends, (lengths << 1) | 1, torch.zeros_like(lengths))
    adv, ret = TL.gae_timelimit(rew, code, V, n, T, 0.99, 0.95, scan=scan)
    a_ref, r_ref = R.gae(rew, (code != 0).to(torch.uint8), V, n, T, 0.99, 0.95, scan=scan)
    assert ends.any() or T * n < 10
    assert torch.equal(adv, a_ref) and torch.equal(ret, r_ref)
    assert TL.end_counts(code) == (0, int(ends.sum()))


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("n,T", [(5, 1), (3, 9), (17, 136), (4, 200)])
def test_no_ends_is_plain_gae_without_dones(n, T, scan):
    rew, V, _, _ = _inputs(n, T, 11 * n + T)
    code = torch.zeros(T * n, dtype=torch.int64)
    adv, ret = TL.gae_timelimit(rew, code, V, n, T, 0.99, 0.95, scan=scan)
    a_ref, r_ref = R.gae(rew, torch.zeros(T * n, dtype=torch.uint8), V, n, T, 0.99, 0.95, scan=scan)
    assert torch.equal(adv, a_ref) and torch.equal(ret, r_ref)
    assert TL.end_counts(code) == (0, 0)


@pytest.mark.parametrize("scan", SCANS)
def test_three_steps_by_hand(scan):
    """One env, T = 3, gamma = 0.5, lambda = 0.5 (gamma lambda = 0.25), every number dyadic.
    r = (1, 2, 4); V = (8, 16, 32 | V_3 = 64); codes: t = 0 none, t = 1 a time limit (length 2,
    code 4), t = 2 a termination (length 1, code 3).
      t = 2: term    -> delta = 4 + 0.5 * 64 * 0 - 32 = -28;  c = 0;     A = -28
      t = 1: timeout -> delta = 2 + 0.5 * 16 * 1 - 16 = -6 (V_1 = 16 stands in for V_2);
                        c = 0;     A = -6
      t = 0: no end  -> delta = 1 + 0.5 * 16 * 1 - 8 = 1;     c = 0.25;  A = 1 + 0.25 * (-6) = -0.5
    ret = A + V = (7.5, 10, 4).  The plain GAE would give delta_1 = 2 - 16 = -14."""
    rew = torch.tensor([1.0, 2.0, 4.0])
    V = torch.tensor([8.0, 16.0, 32.0, 64.0])
    code = torch.tensor([0, 4, 3])
    delta, c = TL.delta_and_c(rew, code, V, 1, 3, 0.5, 0.5)
    assert delta.view(-1).tolist() == [1.0, -6.0, -28.0] and c.view(-1).tolist() == [0.25, 0.0, 0.0]
    adv, ret = TL.gae_timelimit(rew, code, V, 1, 3, 0.5, 0.5, scan=scan)
    assert adv.tolist() == [-0.5, -6.0, -28.0]
    assert ret.tolist() == [7.5, 10.0, 4.0]
    plain, _ = R.gae(rew, (code != 0).to(torch.uint8), V, 1, 3, 0.5, 0.5, scan=scan)
    assert plain.tolist() == [1.0 + 0.25 * -14.0, -14.0, -28.0]
    assert TL.end_counts(code) == (1, 1)


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("n,T,every", [(3, 24, 8), (2, 40, 5), (1, 7, 1)])
def test_stationary_value_has_zero_advantage_under_time_limits(n, T, every, scan):
    """Constant reward r = 1, gamma = 0.5 and V = r / (1 - gamma) = 2 everywhere, the exact value of
    the endless task; every `every`-th step ends an episode at a time limit.  With the bootstrap
    every advantage is exactly 0 (delta = 1 + 0.5 * 2 - 2 at every step, ends included).  The plain
    GAE drops the bootstrap at the ends, delta = 1 - 2 = -gamma V, and the error runs back down
    the chain."""
    gamma, lam, r = 0.5, 0.75, 1.0
    v = r / (1.0 - gamma)
    rew = torch.full((T * n,), r)
    V = torch.full(((T + 1) * n,), v)
    t = torch.arange(T).repeat_interleave(n)
    ends = (t + 1) % every == 0
    code = torch.where(ends, torch.full_like(t, every << 1), torch.zeros_like(t))
    adv, ret = TL.gae_timelimit(rew, code, V, n, T, gamma, lam, scan=scan)
    assert torch.equal(adv, torch.zeros(T * n)) and torch.equal(ret, V[:T * n])
    plain, _ = R.gae(rew, ends.to(torch.uint8), V, n, T, gamma, lam, scan=scan)
    assert ends.any() and torch.equal(plain[ends], torch.full((int(ends.sum()),), -gamma * v))
    assert TL.end_counts(code) == (int(ends.sum()), 0)


def test_config_field_cli_flag_and_checkpoint_entry():
    """TrainerConfig.timeout_bootstrap defaults to False; train --timeout-bootstrap sets it (and is
    refused on a --resume run, which keeps its checkpoint's setting); the checkpoint's
    trainer_config carries the field only when it is set, so a trainer without the option writes the
    entry it always did and an entry without the field loads as the default."""
    import dataclasses

    from dexterous_rl_manipulation_amd import train
    from dexterous_rl_manipulation_amd import training_run as T
    from dexterous_rl_manipulation_amd.trainer import TrainerConfig
    assert TrainerConfig().timeout_bootstrap is False
    base = ["--iterations", "1", "--out", "x"]
    assert train.parse_args(base).timeout_bootstrap is False
    assert train.parse_args(base + ["--timeout-bootstrap"]).timeout_bootstrap is True
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--timeout-bootstrap", "--resume", "ck.npz"])
    assert "timeout_bootstrap" not in T._trainer_config_state(TrainerConfig())
    state = T._trainer_config_state(TrainerConfig(timeout_bootstrap=True))
    assert state["timeout_bootstrap"] is True
    state["betas"] = tuple(state["betas"])
    assert TrainerConfig(**state) == TrainerConfig(timeout_bootstrap=True)
    state.pop("timeout_bootstrap")
    assert TrainerConfig(**state) == TrainerConfig()
    assert dataclasses.asdict(TrainerConfig(**state))["timeout_bootstrap"] is False
