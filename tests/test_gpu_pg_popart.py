"""GPU: dxrl_pg_popart_rescale (csrc/dxrl_pg.hip k_popart_rescale) and the forgetting factor of the
value-normalisation fold (vnorm_fold, behind k_gae_finish and k_vnorm_combine) through ctypes
against the restatement (tests/pg_popart_reference.py).  The rescale kernel has one shape, so its
cases are states."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pg_popart_reference as PA
import pg_vnorm_reference as VN
import test_gpu_pg_vnorm as G  # its helpers: inputs, canaried dxrl_pg_gae_vnorm calls, block words

pytestmark = pytest.mark.gpu

CANARY = 64
F32 = lambda x: float(np.float32(x))  # noqa: E731
# (mu_h, sigma_h) -> (mu_n, sigma_n); mu / sigma of a vnorm block are f32 values widened to f64
RESCALES = {
    "shift": ((1.5, 2.0), (F32(-3.3), 2.0)),
    "scale_up": ((0.0, 1.0), (0.0, F32(7.7))),
    "scale_down": ((F32(2.2), F32(9.1)), (F32(2.2), F32(0.37))),
    "both": ((F32(34.1), F32(10.9)), (F32(35.7), F32(12.3))),
    "ratio_1e3_up": ((F32(0.5), F32(0.02)), (F32(-40.0), F32(20.0))),
    "ratio_1e3_down": ((F32(-40.0), F32(20.0)), (F32(0.5), F32(0.02))),
}
# the forward test's pair: a shift far above what two bf16 roundings of the head can move a value by
PRESERVE = ((F32(34.1), F32(10.9)), (F32(80.3), F32(12.3)))
EQUAL = ((F32(34.1), F32(10.9)), (F32(34.1), F32(10.9)))
REFUSED = {
    "sigma_n_zero": ((1.0, 2.0), (3.0, 0.0)),
    "sigma_n_inf": ((1.0, 2.0), (3.0, math.inf)),
    "mu_n_nan": ((1.0, 2.0), (math.nan, 2.0)),
    "sigma_h_negative": ((1.0, -2.0), (3.0, 2.0)),
}


@pytest.fixture(scope="module")
def N():
    from dexterous_rl_manipulation_amd import _native
    return _native


@pytest.fixture(scope="module")
def T():
    from dexterous_rl_manipulation_amd import trainer
    return trainer


def master(T, seed=0):
    """Random f32 master parameters on the host; the critic head holds zeros and a -0.0."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(T.NPARAMS, generator=g)
    head = p[T.OFF["W3c"]:T.OFF["W3c"] + PA.HEAD]
    head[:256] *= 0.05
    head[3] = 0.0
    head[17] = -0.0
    head[255] = 0.0
    assert torch.signbit(head[17]) and head[17] == 0.0
    return p


def vnorm_block(N, dev, mu, sigma, forget=0.0):
    b = G.prepared_block(N, dev)
    b[N.PG_VNORM["mu"]], b[N.PG_VNORM["sigma"]] = mu, sigma
    b[N.PG_VNORM["batch_count"]], b[N.PG_VNORM["batch_mean"]], b[N.PG_VNORM["batch_m2"]] = 800.0, 33.5, 91000.25
    b[N.PG_VNORM["forget"]] = forget
    return b


def popart_block(N, dev, mu, sigma, rescales=3.0, skipped=1.0):
    b = N.popart_fresh(dev)
    for k, v in (("mu_head", mu), ("sigma_head", sigma), ("rescales", rescales), ("skipped", skipped),
                 ("last_scale", 0.75), ("last_shift", -0.25)):
        b[N.PG_POPART[k]] = v
    return b


def pwords(N, block):
    b = block.tolist()
    return {k: b[i] for k, i in N.PG_POPART.items()}


def same_f64(a, b):
    """Bitwise equality of two lists of Python floats (NaN equals the same NaN)."""
    return np.array(a, dtype=np.float64).tobytes() == np.array(b, dtype=np.float64).tobytes()


class Buffers:
    """params / m1 / m2 / packed with canaries behind them, the pack made by dxrl_pg_pack_weights."""

    def __init__(self, N, T, dev, seed=0):
        host = master(T, seed)
        g = torch.Generator().manual_seed(seed + 1)
        canary = lambda t, v: torch.cat([t, torch.full((CANARY,), v, dtype=t.dtype)]).to(dev)  # noqa: E731
        self.params = canary(host, 7.0)
        self.m1 = canary(torch.randn(T.NPARAMS, generator=g), 7.0)
        self.m2 = canary(torch.rand(T.NPARAMS, generator=g), 7.0)
        self.packed = torch.full((T.NBF + CANARY,), 7.0, dtype=torch.bfloat16, device=dev)
        N.call("dxrl_pg_pack_weights", 0, N.ptr(self.params), N.ptr(self.packed), N.stream_of(dev))
        torch.cuda.synchronize()
        self.before = {k: getattr(self, k).clone() for k in ("params", "m1", "m2", "packed")}

    def repacked(self, N):
        """dxrl_pg_pack_weights of the current master, canary included."""
        out = torch.full_like(self.packed, 7.0)
        N.call("dxrl_pg_pack_weights", 0, N.ptr(self.params), N.ptr(out), N.stream_of(out.device))
        torch.cuda.synchronize()
        return out


def call(N, buf, vn, pa, row):
    a = N.PgPopartArgs()
    a.params, a.packed, a.vnorm, a.popart, a.row_out = N.ptr(buf.params), N.ptr(buf.packed), N.ptr(vn), N.ptr(pa), \
        N.ptr(row)
    N.call("dxrl_pg_popart_rescale", 0, C.byref(a), N.stream_of(buf.params.device))
    torch.cuda.synchronize()
    return a


def bytes_of(t):
    return t.cpu().view(torch.uint8).numpy().tobytes() if t.dtype != torch.bfloat16 else \
        t.cpu().view(torch.int16).numpy().tobytes()


def new_row(N, dev):
    return torch.full((N.PG_VNORM_LOG_COLS + CANARY,), -5.0, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("name", sorted(RESCALES))
def test_rescale_is_the_restatement_and_touches_nothing_else(N, T, name):
    """The 257 master floats, the popart block and the row equal the restatement bit for bit; the
    pack equals dxrl_pg_pack_weights of the new master byte for byte; every other element of
    params, all of m1 / m2, the vnorm block and the canaries keep their bytes."""
    dev = torch.device("cuda", 0)
    (mu_h, sigma_h), (mu_n, sigma_n) = RESCALES[name]
    buf = Buffers(N, T, dev)
    vn, pa, row = vnorm_block(N, dev, mu_n, sigma_n, forget=0.125), popart_block(N, dev, mu_h, sigma_h), new_row(N, dev)
    vn0 = vn.clone()
    lo = T.OFF["W3c"]
    head0 = buf.before["params"][lo:lo + PA.HEAD].cpu().numpy()
    want_head, want_block, want_row = PA.popart_call(head0, pwords(N, pa), G.words(N, vn))
    assert PA.case(mu_h, sigma_h, mu_n, sigma_n) == "rescale"
    call(N, buf, vn, pa, row)
    got = buf.params[lo:lo + PA.HEAD].cpu().numpy()
    assert got.tobytes() == want_head.tobytes()
    assert np.signbit(got[17]) and got[17] == 0.0 and got[3] == 0.0  # zeros keep their signs
    assert same_f64([pwords(N, pa)[k] for k in N.PG_POPART_NAMES], [want_block[k] for k in N.PG_POPART_NAMES])
    assert want_block["rescales"] == 4.0 and want_block["skipped"] == 1.0
    assert all(x == 0.0 for x in pa.tolist()[N.PG_POPART_NAMED:])
    assert same_f64(row[:N.PG_VNORM_LOG_COLS].tolist(), [want_row[k] for k in N.PG_VNORM_LOG_COLUMNS])
    assert want_row["rescaled"] == 1.0 and want_row["forget"] == 0.125
    assert (row[N.PG_VNORM_LOG_COLS:] == -5.0).all()
    expect = buf.before["params"].clone()
    expect[lo:lo + PA.HEAD] = torch.from_numpy(want_head).to(dev)
    assert bytes_of(buf.params) == bytes_of(expect)
    assert bytes_of(buf.m1) == bytes_of(buf.before["m1"]) and bytes_of(buf.m2) == bytes_of(buf.before["m2"])
    assert bytes_of(buf.packed) == bytes_of(buf.repacked(N))
    assert bytes_of(buf.packed) != bytes_of(buf.before["packed"])
    assert torch.equal(vn, vn0)


def test_equal_pairs_write_nothing_but_the_row(N, T):
    dev = torch.device("cuda", 0)
    (mu_h, sigma_h), (mu_n, sigma_n) = EQUAL
    buf = Buffers(N, T, dev, seed=2)
    vn, pa, row = vnorm_block(N, dev, mu_n, sigma_n), popart_block(N, dev, mu_h, sigma_h), new_row(N, dev)
    vn0, pa0 = vn.clone(), pa.clone()
    _, _, want_row = PA.popart_call(np.zeros(PA.HEAD, np.float32), pwords(N, pa), G.words(N, vn))
    call(N, buf, vn, pa, row)
    for k in ("params", "m1", "m2", "packed"):
        assert bytes_of(getattr(buf, k)) == bytes_of(buf.before[k]), k
    assert torch.equal(pa, pa0) and torch.equal(vn, vn0)
    assert same_f64(row[:N.PG_VNORM_LOG_COLS].tolist(), [want_row[k] for k in N.PG_VNORM_LOG_COLUMNS])
    r = dict(zip(N.PG_VNORM_LOG_COLUMNS, row.tolist()))
    assert (r["rescaled"], r["scale"], r["shift"]) == (0.0, 1.0, 0.0) and (r["mu"], r["sigma"]) == (mu_n, sigma_n)
    # a fresh pair against a fresh block, without a row: nothing at all
    vn, pa = N.vnorm_fresh(dev), N.popart_fresh(dev)
    call(N, buf, vn, pa, None)
    assert torch.equal(pa, N.popart_fresh(dev)) and bytes_of(buf.params) == bytes_of(buf.before["params"])
    assert bytes_of(buf.packed) == bytes_of(buf.before["packed"])


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_states_change_only_skipped(N, T, name):
    dev = torch.device("cuda", 0)
    (mu_h, sigma_h), (mu_n, sigma_n) = REFUSED[name]
    assert PA.case(mu_h, sigma_h, mu_n, sigma_n) == "refused"
    buf = Buffers(N, T, dev, seed=3)
    vn, pa, row = vnorm_block(N, dev, mu_n, sigma_n), popart_block(N, dev, mu_h, sigma_h), new_row(N, dev)
    vn0, want = vn.clone(), pwords(N, pa)
    want["skipped"] += 1.0
    call(N, buf, vn, pa, row)
    for k in ("params", "m1", "m2", "packed"):
        assert bytes_of(getattr(buf, k)) == bytes_of(buf.before[k]), k
    assert same_f64([pwords(N, pa)[k] for k in N.PG_POPART_NAMES], [want[k] for k in N.PG_POPART_NAMES])
    assert (row == -5.0).all() and bytes_of(vn) == bytes_of(vn0)


def test_null_pointers_are_refused_before_a_launch(N, T):
    dev = torch.device("cuda", 0)
    (mu_h, sigma_h), (mu_n, sigma_n) = RESCALES["both"]
    buf = Buffers(N, T, dev, seed=4)
    vn, pa = vnorm_block(N, dev, mu_n, sigma_n), popart_block(N, dev, mu_h, sigma_h)
    pa0 = pa.clone()
    fn = N.lib().dxrl_pg_popart_rescale
    for k in ("params", "packed", "vnorm", "popart"):
        a = N.PgPopartArgs()
        a.params, a.packed, a.vnorm, a.popart = N.ptr(buf.params), N.ptr(buf.packed), N.ptr(vn), N.ptr(pa)
        setattr(a, k, None)
        assert fn(0, C.byref(a), N.stream_of(dev)) == N.DXRL_E_INVALID, k
        with pytest.raises(ValueError):
            N.call("dxrl_pg_popart_rescale", 0, C.byref(a), N.stream_of(dev))
    assert fn(0, None, N.stream_of(dev)) == N.DXRL_E_INVALID
    torch.cuda.synchronize()
    assert torch.equal(pa, pa0) and bytes_of(buf.params) == bytes_of(buf.before["params"])
    assert bytes_of(buf.packed) == bytes_of(buf.before["packed"])


def test_decoded_values_survive_the_rescale_through_the_real_forward(N, T):
    """The critic's forward (dxrl_pg_fused, train = 0) over 64 rows of random bf16 observations,
    before and after a rescale of a trainer's own head: sigma_h vn + mu_h against
    sigma_n vn' + mu_n within the derived bound (pg_popart_reference.preservation_bound, from the
    actual weights), which lies far below |mu_h - mu_n| -- without the rescale the decoded values
    would move by about that much."""
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import envs
    dev = torch.device("cuda", 0)
    env = envs.VecEnv(32, curriculum_config=pkg.CurriculumConfig.hard(), reward_type="dense", seed=3, device=dev)
    tr = T.PGTrainer(env, T.TrainerConfig(horizon=1, seed=1, value_norm=True, popart=True))
    rows = tr.M + tr.n
    assert rows == 64
    g = torch.Generator().manual_seed(11)
    obs = torch.zeros(rows, T.IN)
    obs[:, :T.OBS_IN] = torch.randn(rows, T.OBS_IN, generator=g)
    obs[:, T.OBS_IN] = 1.0  # the bias column
    tr.obs_rm.copy_(obs.to(torch.bfloat16).to(dev))
    (mu_h, sigma_h), (mu_n, sigma_n) = PRESERVE
    tr.popart.copy_(popart_block(N, dev, mu_h, sigma_h))
    tr.vnorm[N.PG_VNORM["mu"]], tr.vnorm[N.PG_VNORM["sigma"]] = mu_n, sigma_n
    lo = T.OFF["W3c"]
    head = tr.params[lo:lo + PA.HEAD].cpu().numpy()
    tr.critic_values()
    torch.cuda.synchronize()
    before = sigma_h * tr.V[0].double().cpu().numpy() + mu_h
    tr.popart_rescale()
    tr.critic_values()
    torch.cuda.synchronize()
    after = sigma_n * tr.V[0].double().cpu().numpy() + mu_n
    assert tr.popart_state()["rescales"] == 4 and tr.popart_state()["mu_head"] == mu_n
    bound = PA.preservation_bound(head, mu_h, sigma_h, mu_n)
    err = np.abs(after - before).max()
    print(f"decoded values moved by at most {err:.3e}; bound {bound:.3e}; |mu_h - mu_n| = {abs(mu_h - mu_n):.3e}")
    assert bound < abs(mu_h - mu_n) / 16.0
    assert err <= bound
    assert np.abs(before).max() > 1.0 and np.ptp(before) > 0.0  # the forward ran on real values


# ---------------------------------------------------------------------------- forgetting
FORGET = 0.25


@pytest.mark.parametrize("n,T_", [(1, 1), (17, 9), (65, 601)])
def test_forgetting_through_gae_vnorm_two_folds(N, n, T_):
    """A non-zero FORGET word, two folds on one block (k_gae_lds with a ragged last workgroup, and
    k_gae past the LDS horizon): the running triple and (mu, sigma) after each fold are
    fold_forget's of the batch triple the call wrote, bit for bit; FORGET is never written."""
    dev = torch.device("cuda", 0)
    block = N.vnorm_fresh(dev)
    block[N.PG_VNORM["forget"]] = FORGET
    state = VN.fresh_state()
    for k in range(2):
        rew_h, V_h, done_h, _ = G.data(n, T_, 31 * n + T_ + k, 1.0)
        G.run_vnorm(N, "done", rew_h.to(dev), done_h.to(dev), V_h.to(dev), n, T_, block)
        w = G.words(N, block)
        state = PA.fold_forget(state, G.triple(w, "batch_"), G.EPS, FORGET)
        assert G.running(w) == state["running"], (k, G.running(w), state["running"])
        assert (w["mu"], w["sigma"], w["calls"]) == (state["mu"], state["sigma"], k + 1.0)
        assert w["forget"] == FORGET
    assert state["running"][0] == (1.0 - FORGET) * n * T_ + n * T_
    assert all(x == 0.0 for x in block.tolist()[N.PG_VNORM_NAMED:])


@pytest.mark.parametrize("world", sorted(G.ROWS))
def test_forgetting_through_vnorm_combine(N, world):
    """Hand-made ranks (one of them empty): the fold behind the rank-order merge discounts the
    running triple first; FORGET stays."""
    dev = torch.device("cuda", 0)
    rows = torch.tensor(G.ROWS[world], dtype=torch.float64)
    block = G.prepared_block(N, dev)
    block[N.PG_VNORM["forget"]] = FORGET
    w0 = G.words(N, block)
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    N.call("dxrl_pg_vnorm_combine", 0, N.ptr(rows.to(dev)), world, N.ptr(stats), N.ptr(block), N.stream_of(dev))
    torch.cuda.synchronize()
    w = G.words(N, block)
    batch = VN.merge_rows(rows[:, :3].tolist())
    want = PA.fold_forget({"running": G.running(w0), "mu": w0["mu"], "sigma": w0["sigma"], "calls": 5}, batch, G.EPS,
                          FORGET)
    assert G.running(w) == want["running"] and (w["mu"], w["sigma"]) == (want["mu"], want["sigma"])
    assert w["calls"] == 6.0 and w["forget"] == FORGET
    assert G.running(w) != VN.fold({"running": G.running(w0), "mu": w0["mu"], "sigma": w0["sigma"], "calls": 5},
                                   batch, G.EPS)["running"]
