"""CPU: the manual PG backward (pg_reference.py, mirrored by the HIP kernels)
equals torch autograd on the same PPO + value + entropy objective (fp64)."""
import pytest
import torch

import pg_reference as R


def make_case(n=8, T=6, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    params = torch.zeros(R.NPARAMS, dtype=dtype)
    Wd = R.unpack(params)
    for net in "ac":
        Wd[f"W1{net}"][:, :R.OBS_IN + 1] = 0.2 * torch.randn(R.H, R.OBS_IN + 1, generator=g, dtype=dtype)
        Wd[f"W2{net}"][:, :R.H + 1] = 0.08 * torch.randn(R.H, R.H + 1, generator=g, dtype=dtype)
        rows = R.ACT if net == "a" else 1
        Wd[f"W3{net}"][:rows, :R.H + 1] = 0.1 * torch.randn(rows, R.H + 1, generator=g, dtype=dtype)
    Wd["logstd"][:] = -0.5 + 0.1 * torch.randn(R.ACT, generator=g, dtype=dtype)
    obs = torch.zeros((T + 1) * n, R.IN, dtype=dtype)
    obs[:, :R.OBS_IN] = torch.randn((T + 1) * n, R.OBS_IN, generator=g, dtype=dtype)
    obs[:, R.OBS_IN] = 1.0
    M = n * T
    act = torch.zeros(M, 16, dtype=dtype)
    act[:, :R.ACT] = torch.randn(M, R.ACT, generator=g, dtype=dtype)
    rew = torch.rand(M, generator=g, dtype=dtype)
    done = (torch.rand(M, generator=g) < 0.15).to(torch.uint8)
    with torch.no_grad():
        _, _, mh = R.mlp_forward(obs[:M], R.unpack(params), "a", False)
        mu, ls = mh[:, :R.ACT], R.unpack(params)["logstd"]
        lp = (-0.5 * ((act[:, :R.ACT] - mu) * torch.exp(-ls)) ** 2 - ls - 0.5 * R.LOG2PI).sum(1)
    logp_old = lp + 0.3 * torch.randn(M, generator=g, dtype=dtype)  # ratios != 1: clipping active
    return params, obs, act, logp_old, rew, done


CFG = dict(gamma=0.99, lam=0.95, clip_eps=0.2, vf_coef=0.5, ent_coef=0.01)


def test_manual_backward_matches_autograd():
    n, T = 8, 6
    params, obs, act, logp_old, rew, done = make_case(n, T)
    grads, info = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, CFG, bf16=False)
    ref = R.autograd_loss(params, obs, act, logp_old, rew, done, n, T, CFG)
    assert ((info["ratio"] - 1).abs() > CFG["clip_eps"]).any()  # the clipped branch is exercised
    torch.testing.assert_close(grads, ref, rtol=1e-9, atol=1e-12)


def test_gae_matches_closed_form_single_episode():
    n, T, gamma, lam = 1, 5, 0.9, 0.8
    rew = torch.arange(1, T + 1, dtype=torch.float64)
    done = torch.zeros(T, dtype=torch.uint8)
    V = torch.linspace(0.5, 1.5, T + 1, dtype=torch.float64)
    adv, ret = R.gae(rew, done, V, n, T, gamma, lam)
    deltas = rew + gamma * V[1:] - V[:-1]
    expect = torch.tensor([sum((gamma * lam) ** (k - t) * deltas[k] for k in range(t, T)) for t in range(T)],
                          dtype=torch.float64)
    torch.testing.assert_close(adv, expect)
    torch.testing.assert_close(ret, expect + V[:-1])
    done[2] = 1  # episode boundary cuts the bootstrap and the trace
    adv2, _ = R.gae(rew, done, V, n, T, gamma, lam)
    assert abs(adv2[2] - (rew[2] - V[2])) < 1e-12


@pytest.mark.parametrize("n,T,p_done", [(7, 1, 0.0), (5, 9, 0.2), (33, 200, 0.02), (4, 129, 0.0), (3, 600, 0.05)])
def test_gae_segmented_scan_equals_sequential_recurrence(n, T, p_done):
    """k_gae_lds's segmented scan (restated op for op by pg_reference.gae) against the one-chain
    f32 recurrence and an f64 one: the composition only re-rounds each segment's incoming value, so
    the two f32 forms agree to a few ulp of the chain's magnitude and both sit within 1e-5 of f64
    (north star: returns within 1e-5)."""
    g = torch.Generator().manual_seed(1000 * n + T)
    rew = torch.randn(T * n, generator=g)
    V = torch.randn((T + 1) * n, generator=g) * 3.0
    done = (torch.rand(T * n, generator=g) < p_done).to(torch.uint8)
    a_scan, r_scan = R.gae(rew, done, V, n, T, 0.99, 0.95, scan=True)
    a_seq, r_seq = R.gae(rew, done, V, n, T, 0.99, 0.95, scan=False)
    a64, _ = R.gae(rew.double(), done, V.double(), n, T, 0.99, 0.95, scan=False)
    scale = a64.abs().max().item() + 1.0
    assert (a_scan.double() - a_seq.double()).abs().max().item() <= 1e-6 * scale
    assert (a_scan.double() - a64).abs().max().item() <= 1e-5 * scale
    torch.testing.assert_close(r_scan, a_scan + V.view(T + 1, n)[:T].reshape(-1), rtol=0, atol=0)
    if T <= 8:  # one chunk: a single segment holds the whole horizon, no composition at all
        assert torch.equal(a_scan, a_seq)


def test_fp64_pin_ratios():
    """pg_reference.fp64_pin: the bf16-emulating reference itself sits at ratio 1 of its own
    distance to the fp64 truth; a result with doubled error (got = truth + 2 (ref - truth))
    is rejected."""
    import pytest
    n, T = 8, 6
    params, obs, act, logp_old, rew, done = make_case(n, T, dtype=torch.float32)
    logp_old = logp_old.float()
    g, info = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, CFG, bf16=True)
    r = R.fp64_pin(g, info["V"], info["adv"], params, obs, act, logp_old, rew, done, n, T, CFG, g, info)
    assert all(abs(v - 1.0) < 1e-6 for v in r.values()), r
    g64, info64 = R.loss_and_grads(params.double(), obs, act, logp_old, rew, done, n, T, CFG, bf16=False)
    worse = g.double() + (g.double() - g64)
    with pytest.raises(AssertionError):
        R.fp64_pin(worse, info["V"], info["adv"], params, obs, act, logp_old, rew, done, n, T, CFG, g, info)


# ---------------------------------------------------------------- off-policy / trained-like additions
def synthetic_tape(n, T, seed, params, dtype=torch.float32):
    """A tape as the rollout would leave it under `params`: bf16-valued observations with the ones
    column, actions sampled from the policy (fp64 forward), their log-probabilities, rewards, dones."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.zeros((T + 1) * n, R.IN, dtype=torch.float64)
    obs[:, :R.OBS_IN] = torch.randn((T + 1) * n, R.OBS_IN, generator=g, dtype=torch.float64).clamp(-3, 3)
    obs = obs.to(torch.bfloat16).double()
    obs[:, R.OBS_IN] = 1.0
    M = n * T
    Wd = R.unpack(params.double())
    _, _, mh = R.mlp_forward(obs[:M], Wd, "a", False)
    mu, ls = mh[:, :R.ACT], Wd["logstd"]
    act = torch.zeros(M, 16, dtype=torch.float64)
    act[:, :R.ACT] = mu + torch.exp(ls) * torch.randn(M, R.ACT, generator=g, dtype=torch.float64)
    lp = (-0.5 * ((act[:, :R.ACT] - mu) * torch.exp(-ls)) ** 2 - ls - 0.5 * R.LOG2PI).sum(1)
    rew = torch.rand(M, generator=g, dtype=torch.float64)
    done = (torch.rand(M, generator=g) < 0.1).to(torch.uint8)
    return obs.to(dtype), act.to(dtype), lp.to(dtype), rew.to(dtype), done


def test_trained_like_params_layout():
    """No degenerate entry left where the kernels read one: every bias nonzero and within its
    range, 15 distinct log_std, the padding (W1 columns 46.., W2 columns 257.., the head's dead
    rows) still zero, the critic's hidden layers built like the actor's."""
    p = R.trained_like_params(7)
    assert p.shape == (R.NPARAMS,) and p.dtype == torch.float32
    assert torch.equal(p, R.trained_like_params(7)) and not torch.equal(p, R.trained_like_params(8))
    Wd = R.unpack(p)
    for net, rows in (("a", R.ACT), ("c", 1)):
        W1, W2, W3 = Wd[f"W1{net}"], Wd[f"W2{net}"], Wd[f"W3{net}"]
        for b, lim in ((W1[:, R.OBS_IN], 0.1), (W2[:, R.H], 0.1), (W3[:rows, R.H], 0.3)):
            assert (b != 0).all() and b.abs().max() <= lim
        assert W1[:, R.OBS_IN + 1:].abs().sum() == 0 and W2[:, R.H + 1:].abs().sum() == 0
        assert W3[rows:].abs().sum() == 0 and W3[:, R.H + 1:].abs().sum() == 0
        # orthogonal init: W W^T = gain^2 I on the smaller side
        torch.testing.assert_close(W1[:, :R.OBS_IN].T @ W1[:, :R.OBS_IN], 2.0 * torch.eye(R.OBS_IN), atol=1e-4, rtol=0)
        gain = 0.5 if net == "a" else 1.0
        torch.testing.assert_close(W3[:rows, :R.H] @ W3[:rows, :R.H].T, gain ** 2 * torch.eye(rows), atol=1e-4, rtol=0)
    torch.testing.assert_close(Wd["logstd"], torch.linspace(-1.0, -0.2, R.ACT))
    assert p[R.OFF["logstd"] + R.ACT:R.OFF["W1c"]].abs().sum() == 0


@pytest.mark.parametrize("rows", [(0, 48), (16, 24), (37, 11)])
def test_manual_backward_with_rows_matches_autograd_on_the_slice(rows):
    """rows = (start, count): the gradient of the mean loss over that slice alone (scale 1 / count),
    with GAE and the advantage moments over the whole tape, equals autograd in fp64 -- with
    clipping active on both sides, nonzero biases and 15 distinct log_std."""
    n, T = 8, 6
    params = R.trained_like_params(3).double()
    obs, act, lp, rew, done = synthetic_tape(n, T, 5, params, torch.float64)
    logp_old = R.offpolicy_logp(lp, CFG["clip_eps"], 9)
    grads, info = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, CFG, bf16=False, rows=rows)
    ref = R.autograd_loss(params, obs, act, logp_old, rew, done, n, T, CFG, rows=rows)
    torch.testing.assert_close(grads, ref, rtol=1e-9, atol=1e-12)
    assert (info["ratio"] > 1 + CFG["clip_eps"]).any() and (info["ratio"] < 1 - CFG["clip_eps"]).any()
    assert all(v.shape == (rows[1],) for v in info["terms"].values())
    # the moments are the whole tape's, and the slice's terms are the full pass's terms on those rows
    g_all, info_all = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, CFG, bf16=False)
    assert info["mean"] == info_all["mean"] and info["std"] == info_all["std"]
    assert torch.equal(info["adv"], info_all["adv"]) and info["V"].shape == ((T + 1) * n,)
    sl = slice(rows[0], rows[0] + rows[1])
    for k in info["terms"]:
        torch.testing.assert_close(info["terms"][k], info_all["terms"][k][sl], rtol=1e-12, atol=1e-14)
    if rows == (0, n * T):
        torch.testing.assert_close(grads, g_all, rtol=1e-12, atol=1e-15)


def test_row_slices_weight_to_the_full_batch():
    """sum_k rows_k / M x grad_k over a partition == the full-batch gradient (fp64), entropy term
    included: every slice carries the bonus once."""
    n, T = 8, 6
    M = n * T
    params = R.trained_like_params(3).double()
    obs, act, lp, rew, done = synthetic_tape(n, T, 5, params, torch.float64)
    logp_old = R.offpolicy_logp(lp, CFG["clip_eps"], 9)
    g_all, _ = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, CFG, bf16=False)
    acc = torch.zeros_like(g_all)
    for rows in ((0, 10), (10, 27), (37, 11)):
        g, _ = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, CFG, bf16=False, rows=rows)
        acc += rows[1] / M * g
    torch.testing.assert_close(acc, g_all, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("bf16", [False, True])
def test_per_sample_terms_average_to_the_loss(bf16):
    """info["terms"]: policy / value average to the loss (with the closed-form entropy), clip is
    the indicator |ratio - 1| > eps, kl is logp_old - lp; checked against an independent
    restatement from info's own ratio / A / V / ret."""
    n, T = 8, 6
    dt = torch.float32 if bf16 else torch.float64
    params = R.trained_like_params(4).to(dt)
    obs, act, lp, rew, done = synthetic_tape(n, T, 6, params, dt)
    logp_old = R.offpolicy_logp(lp, CFG["clip_eps"], 2)
    _, info = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, CFG, bf16=bf16)
    t = info["terms"]
    ent = R.unpack(params)["logstd"].sum() + 0.5 * R.ACT * (1 + R.LOG2PI)
    loss = t["policy"].mean() + CFG["vf_coef"] * t["value"].mean() - CFG["ent_coef"] * ent
    torch.testing.assert_close(loss, info["loss"], rtol=1e-6, atol=1e-7)
    M, eps = n * T, CFG["clip_eps"]
    r, A = info["ratio"], info["A"]
    want = torch.where(A > 0, -torch.clamp(r, max=1 + eps) * A, -torch.clamp(r, min=1 - eps) * A)
    torch.testing.assert_close(t["policy"], want, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(t["value"], (info["V"][:M] - info["ret"]) ** 2)
    assert t["clip"].dtype == torch.bool and torch.equal(t["clip"], (r > 1 + eps) | (r < 1 - eps))
    torch.testing.assert_close(t["kl"], -torch.log(r), rtol=1e-4, atol=1e-5)
    assert 0.3 < t["clip"].double().mean() < 0.7 and t["kl"].mean() > 0.02


@pytest.mark.parametrize("eps", [0.1, 0.2])
def test_offpolicy_logp_covers_both_sides_of_both_boundaries(eps):
    """offpolicy_logp: all four combinations of advantage sign and clipped side hold >= 5 % of the
    samples; the offsets alone keep >= 0.07 from both boundaries (log space), as does the fp64
    reference's ratio on the tape the offsets were applied to; half inside, half outside; 65 / 35
    signs; only the old log-probabilities change."""
    n, T = 64, 16
    M = n * T
    params = R.trained_like_params(1).double()
    obs, act, lp, rew, done = synthetic_tape(n, T, 11, params, torch.float64)
    cfg = dict(CFG, clip_eps=eps)
    logp_old = R.offpolicy_logp(lp, eps, 4)
    assert torch.equal(logp_old, R.offpolicy_logp(lp, eps, 4)) and logp_old.dtype == lp.dtype
    pert = logp_old - lp
    hi, lo = R.clip_bounds(eps)
    assert hi == pytest.approx(torch.log(torch.tensor(1 + eps, dtype=torch.float64)).item())
    assert lo == pytest.approx(-torch.log(torch.tensor(1 - eps, dtype=torch.float64)).item())
    d = torch.minimum((-pert - hi).abs(), (-pert + lo).abs())  # log ratio = -pert
    assert d.min() >= 0.07
    inside = pert.abs() < hi
    assert (pert.abs()[inside] <= hi - 0.08 + 1e-12).all()
    out = pert.abs()[~inside]
    assert (out >= lo + 0.08 - 1e-12).all() and (out <= lo + 0.7 + 1e-12).all()
    assert 0.45 < inside.double().mean() < 0.55 and 0.60 < (pert > 0).double().mean() < 0.70
    _, info = R.loss_and_grads(params, obs, act, logp_old, rew, done, n, T, cfg, bf16=False)
    assert R.ratio_margin(info, eps) >= 0.07
    assert R.ratio_margin(info, eps) == pytest.approx(d.min().item(), abs=1e-9)
    q = R.clip_quadrants(info, eps)
    assert len(q) == 4 and all(v >= 0.05 for v in q.values()), q
    assert sum(q.values()) == pytest.approx(info["terms"]["clip"].double().mean().item())
    assert int(info["terms"]["clip"].sum()) == int((~inside).sum())
    # the bf16 restatement, whose log pi is off by up to ~0.02 at head gain 0.5, keeps 0.04
    p32 = params.float()
    _, info_b = R.loss_and_grads(p32, obs.float(), act.float(), logp_old.float(), rew.float(), done, n, T, cfg)
    assert R.ratio_margin(info_b, eps) >= 0.04
    assert (info_b["lp"].double() - info["lp"]).abs().max() < 0.04
    assert torch.equal(info_b["terms"]["clip"], info["terms"]["clip"])


def test_ratio_margin_is_the_distance_to_the_nearer_boundary():
    eps = 0.2
    hi, lo = R.clip_bounds(eps)
    lr = torch.tensor([0.0, hi - 0.03, hi + 0.05, -lo + 0.02, -lo - 0.5], dtype=torch.float64)
    info = {"lp": lr, "logp_old": torch.zeros_like(lr)}
    assert R.ratio_margin(info, eps) == pytest.approx(0.02)
    assert R.ratio_margin({"lp": lr[:3], "logp_old": torch.zeros(3, dtype=torch.float64)}, eps) == pytest.approx(0.03)


def test_fp64_pin_bias_columns_logstd_and_logp():
    """fp64_pin's added quantities: the six bias columns and logstd are pinned on their own (an
    error confined to one bias column passes the whole-block pin and fails the column's), the
    optional log pi triple likewise, `rows=` pins a minibatch slice, `factors=` raises the bound
    for the named quantity alone."""
    n, T = 8, 6
    params = R.trained_like_params(2)
    obs, act, lp, rew, done = synthetic_tape(n, T, 3, params)
    logp_old = R.offpolicy_logp(lp, CFG["clip_eps"], 1)
    rows = (16, 24)
    args = (params, obs, act, logp_old, rew, done, n, T, CFG)
    g, info = R.loss_and_grads(*args, bf16=True, rows=rows)
    g64, info64 = R.loss_and_grads(params.double(), *args[1:], bf16=False, rows=rows)
    triple = (info["lp"], info["lp"], info64["lp"])
    r = R.fp64_pin(g, info["V"], info["adv"], *args, g, info, blocks=R.ALL_BLOCKS, rows=rows, logp=triple)
    assert set(r) == set(R.ALL_BLOCKS) | {"V", "adv", "logp"} and len(R.ALL_BLOCKS) == 13
    assert all(abs(v - 1.0) < 1e-6 for v in r.values()), r
    r2 = R.fp64_pin(g, info["V"], info["adv"], *args, g, info, blocks=R.ALL_BLOCKS, rows=rows, truth=(g64, info64))
    assert all(r2[k] == r[k] for k in r2)
    for name in R.BIAS_BLOCKS:
        worse = g.clone()
        col = R.pin_block(worse, name)
        col += 2.0 * (col.double() - R.pin_block(g64, name)).float()  # 3 x the column's error
        blk = R.BIAS_BLOCKS[name][0]
        R.fp64_pin(worse, info["V"], info["adv"], *args, g, info, rows=rows)  # the blocks alone: passes
        with pytest.raises(AssertionError) as e:
            R.fp64_pin(worse, info["V"], info["adv"], *args, g, info, blocks=R.ALL_BLOCKS, rows=rows)
        assert [b[0] for b in e.value.args[0][0]] == [name], (name, blk, e.value.args[0][0])
        rr = R.fp64_pin(worse, info["V"], info["adv"], *args, g, info, blocks=R.ALL_BLOCKS, rows=rows,
                        factors={name: 3.1})
        assert rr[name] == pytest.approx(3.0, rel=1e-3)
    worse = g.clone()
    ls = R.pin_block(worse, "logstd")
    ls += (ls.double() - R.pin_block(g64, "logstd")).float()
    with pytest.raises(AssertionError):
        R.fp64_pin(worse, info["V"], info["adv"], *args, g, info, blocks=("logstd",), rows=rows)
    bad_lp = info["lp"].double() + (info["lp"].double() - info64["lp"])
    with pytest.raises(AssertionError):
        R.fp64_pin(g, info["V"], info["adv"], *args, g, info, rows=rows, logp=(bad_lp, info["lp"], info64["lp"]))


def test_reference_mutations_are_caught(monkeypatch):
    """The checks above have teeth: a reference with the clip branch's inequality flipped, or with
    b2 dropped from the forward, or with logstd read through a wrong row map, no longer matches
    autograd / its own per-sample terms."""
    n, T = 8, 6
    params = R.trained_like_params(3).double()
    obs, act, lp, rew, done = synthetic_tape(n, T, 5, params, torch.float64)
    logp_old = R.offpolicy_logp(lp, CFG["clip_eps"], 9)
    args = (params, obs, act, logp_old, rew, done, n, T, CFG)
    want = R.autograd_loss(*args)
    torch.testing.assert_close(R.loss_and_grads(*args, bf16=False)[0], want, rtol=1e-9, atol=1e-12)

    def differs():
        g, _ = R.loss_and_grads(*args, bf16=False)
        return not torch.allclose(g, want, rtol=1e-6, atol=1e-9)

    real_where = torch.where
    # `<=` to `>=` in gsel: the gradient flows through exactly the wrong samples
    monkeypatch.setattr(R.torch, "where", lambda c, a, b: real_where(~c, a, b))
    assert differs()
    monkeypatch.undo()
    real_fwd = R.mlp_forward

    def no_b2(X, Wd, net, bf16):
        Wd = dict(Wd)
        W2 = Wd[f"W2{net}"].clone()
        W2[:, R.H] = 0
        Wd[f"W2{net}"] = W2
        return real_fwd(X, Wd, net, bf16)

    monkeypatch.setattr(R, "mlp_forward", no_b2)
    assert differs()
    monkeypatch.undo()
    real_unpack = R.unpack

    def swapped_logstd(p):
        out = real_unpack(p)
        if not p.requires_grad:  # the manual pass alone
            out["logstd"] = out["logstd"][[0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14]]
        return out

    monkeypatch.setattr(R, "unpack", swapped_logstd)
    assert differs()
