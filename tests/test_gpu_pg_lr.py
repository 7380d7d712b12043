"""dxrl_pg_adam_step_ctl on the device, through ctypes: random f32 master / gradient / moments of
the real parameter count, crafted partials.

The KL partials are multiples of 2^-20 of bounded size, so their f64 sum is exact in any order
and the restatement (tests/pg_lr_reference.py) needs no knowledge of the kernel's summation
order; every later controller operation is one IEEE f64 operation, so state and rows are
compared bit for bit.  With target_kl = 2^-7, stop_factor 1.5 and 1024 rows the stop threshold
is a KL sum of exactly 12."""
import ctypes as C
import math
import random

import pytest
import torch

import pg_lr_reference as R

pytestmark = pytest.mark.gpu

COUNTS = (1, 4, 255, 256, 257, 2600)  # 2600: the batches-of-8 path of block_sum_partials
STEPS = (1, 2, 7, 100, 5000)
Q = 2.0 ** -20
TARGET, ROWS, AT_THRESHOLD = 2.0 ** -7, 1024, 12.0
BETAS, EPS, MAX_NORM, LR = (0.9, 0.999), 1e-5, 0.5, 3e-4


@pytest.fixture(scope="module")
def N():
    from dexterous_rl_manipulation_amd import _native
    return _native


@pytest.fixture(scope="module")
def sizes():
    from dexterous_rl_manipulation_amd import trainer
    return trainer.NPARAMS, trainer.NBF


@pytest.fixture(scope="module")
def data(sizes):
    """Random inputs shared by the tests (never written: every call writes fresh outputs)."""
    n, _ = sizes
    gen = torch.Generator(device="cuda").manual_seed(21)
    rnd = lambda sd: torch.randn(n, generator=gen, device="cuda") * sd  # noqa: E731
    return {"p": rnd(0.1), "m1": rnd(1e-3), "m2": rnd(1e-3).square(), "g_small": rnd(1e-5), "g_big": rnd(10.0)}


def kl_table(nb, kl_sum, seed=0):
    """f64 [nb][4] loss partials whose column 3 sums to kl_sum exactly in any order (multiples of
    2^-20, both signs); the other columns hold values a wrong stride or column would pick up."""
    rng = random.Random(seed * 7919 + nb)
    units = round(kl_sum / Q)
    assert units * Q == kl_sum
    col = [rng.randrange(-2 ** 22, 2 ** 22) for _ in range(nb - 1)]
    col.append(units - sum(col))
    t = torch.full((nb, 4), 1e6, dtype=torch.float64)
    t[:, 3] = torch.tensor(col, dtype=torch.float64) * Q
    return t.cuda()


def gn_partials(nb, g):
    """nb positive f64 partials whose sum is about the gradient's squared norm."""
    w = torch.rand(nb, dtype=torch.float64, generator=torch.Generator().manual_seed(nb)) + 0.5
    return (w / w.sum() * float(g.double().square().sum())).cuda()


def state_tensor(read_slot_state, calls):
    """A device state block whose slot read by call number `calls` holds the given state; the
    other slot holds a pattern the call must overwrite."""
    words = [[-7] * R.SLOT_WORDS, [-7] * R.SLOT_WORDS]
    words[(calls - 1) & 1] = R.state_words(read_slot_state)
    return torch.tensor(words, dtype=torch.int64).cuda()


class Out:
    def __init__(self, sizes, sentinel=False):
        n, nbf = sizes
        self.p, self.m1, self.m2 = (torch.full((n,), float("nan"), device="cuda") for _ in range(3))
        self.g2 = torch.zeros(1, dtype=torch.float64, device="cuda")
        self.packed = torch.zeros(nbf, dtype=torch.bfloat16, device="cuda")
        if sentinel:
            self.packed.view(torch.int16).fill_(0x5A5A)

    def same(self, o):
        return (torch.equal(self.p, o.p) and torch.equal(self.m1, o.m1) and torch.equal(self.m2, o.m2)
                and torch.equal(self.g2, o.g2) and torch.equal(self.packed.view(torch.int16), o.packed.view(torch.int16)))


def parent(N, sizes, inp, g, step, lr=LR, gn=None, max_norm=MAX_NORM):
    """dxrl_pg_adam_step on the partials gn, or (gn None) dxrl_pg_optimizer_step."""
    o = Out(sizes)
    p = N.ptr
    args = (0, p(inp["p"]), p(g), p(inp["m1"]), p(inp["m2"]), p(o.p), p(o.m1), p(o.m2), sizes[0], lr, BETAS[0], BETAS[1],
            EPS, step, max_norm)
    if gn is None:
        scratch = torch.zeros(512, dtype=torch.float64, device="cuda")
        N.call("dxrl_pg_optimizer_step", *args, p(scratch), p(o.g2), p(o.packed), None)
    else:
        N.call("dxrl_pg_adam_step", *args, p(gn), gn.numel(), p(o.g2), p(o.packed), None)
    return o


def ctl(N, sizes, inp, g, state, calls, kl, rows=ROWS, gn=None, max_norm=MAX_NORM, out=None, row=None, **kw):
    """One dxrl_pg_adam_step_ctl call; kw: the fields of R.control."""
    c = R.control(**dict(dict(lr_nominal=LR), **kw))
    k = N.PgLrControl(calls=calls, **c)
    o = out or Out(sizes)
    p = N.ptr
    scratch = torch.zeros(512, dtype=torch.float64, device="cuda") if gn is None else gn
    N.call("dxrl_pg_adam_step_ctl", 0, p(inp["p"]), p(g), p(inp["m1"]), p(inp["m2"]), p(o.p), p(o.m1), p(o.m2), sizes[0],
           BETAS[0], BETAS[1], EPS, max_norm, p(scratch), 0 if gn is None else gn.numel(), p(o.g2), p(o.packed),
           p(kl), kl.shape[0], rows, k, p(state), p(row), None)
    return o, c


def slot(state, calls):
    torch.cuda.synchronize()
    return state[calls & 1].cpu().tolist()


def advanced(applied):
    s = R.fresh_state()
    s["applied"] = applied
    return s


# ------------------------------------------------------------------ inert controller == parent
@pytest.mark.parametrize("nb", COUNTS)
def test_inert_controller_equals_adam_step(N, sizes, data, nb):
    """target_kl = 0, scale 1, never skipped: master, moments, gnorm2 and every bf16 of the pack
    are dxrl_pg_adam_step's at the same t, for every partial count (of the norm and of the loss
    rows), clip engaged and not.  The KL column is far above any threshold: no rule is on."""
    kl = kl_table(nb, 4096.0)
    for g in (data["g_small"], data["g_big"]):
        gn = gn_partials(nb, g)
        for t in STEPS:
            want = parent(N, sizes, data, g, t, gn=gn)
            st = state_tensor(advanced(t - 1), t)
            got, c = ctl(N, sizes, data, g, st, t, kl, gn=gn)
            assert got.same(want), (nb, t)
            ref, d, _ = R.step(advanced(t - 1), c, 4096.0, ROWS)
            assert d["applied"] and d["t"] == t and slot(st, t) == R.state_words(ref), (nb, t)


def test_inert_controller_equals_optimizer_step_on_the_sumsq_route(N, sizes, data):
    kl = kl_table(4, 0.0)
    for g, clipped in ((data["g_small"], False), (data["g_big"], True)):
        assert (float(g.double().square().sum()) ** 0.5 > MAX_NORM) == clipped
        for t in STEPS:
            want = parent(N, sizes, data, g, t)
            got, _ = ctl(N, sizes, data, g, state_tensor(advanced(t - 1), t), t, kl)
            assert got.same(want), t
    # and without clipping at all
    want = parent(N, sizes, data, data["g_big"], 3, max_norm=0.0)
    got, _ = ctl(N, sizes, data, data["g_big"], state_tensor(advanced(2), 3), 3, kl, max_norm=0.0)
    assert got.same(want)


# ------------------------------------------------------------------ stop
@pytest.mark.parametrize("nb", COUNTS)
def test_stop_is_strict_and_copies_through(N, sizes, data, nb):
    g = data["g_small"]
    gn = gn_partials(nb, g)
    kw = dict(target_kl=TARGET, stop_factor=1.5, last_epoch=0, last_pass=0)
    # exactly at stop_factor x target_kl: applied, the parent's bytes
    st = state_tensor(R.fresh_state(), 1)
    got, c = ctl(N, sizes, data, g, st, 1, kl_table(nb, AT_THRESHOLD), gn=gn, pass_index=0, **kw)
    assert got.same(parent(N, sizes, data, g, 1, gn=gn))
    s1, d, _ = R.step(R.fresh_state(), c, AT_THRESHOLD, ROWS)
    assert d["applied"] and slot(st, 1) == R.state_words(s1)
    # one 2^-20 above, as pass 1: outputs == inputs bit for bit, the pack keeps the sentinel
    o = Out(sizes, sentinel=True)
    ctl(N, sizes, data, g, st, 2, kl_table(nb, AT_THRESHOLD + Q), gn=gn, out=o, pass_index=1, **kw)
    s2, d, _ = R.step(s1, R.control(LR, pass_index=1, **kw), AT_THRESHOLD + Q, ROWS)
    assert not d["applied"] and slot(st, 2) == R.state_words(s2) and s2["stop_pass"] == 1
    assert torch.equal(o.p, data["p"]) and torch.equal(o.m1, data["m1"]) and torch.equal(o.m2, data["m2"])
    assert bool((o.packed.view(torch.int16) == 0x5A5A).all())
    assert float(o.g2) == float(gn_sum_of(N, sizes, data, g, gn))  # the norm is still reported
    # a later pass with KL 0 still copies through
    o = Out(sizes, sentinel=True)
    ctl(N, sizes, data, g, st, 3, kl_table(nb, 0.0), gn=gn, out=o, pass_index=2, **kw)
    s3, d, _ = R.step(s2, R.control(LR, pass_index=2, **kw), 0.0, ROWS)
    assert not d["applied"] and slot(st, 3) == R.state_words(s3) and s3["skipped"] == 2
    assert torch.equal(o.p, data["p"]) and bool((o.packed.view(torch.int16) == 0x5A5A).all())
    # pass_index 0 applies again
    o, c = ctl(N, sizes, data, g, st, 4, kl_table(nb, 0.0), gn=gn, pass_index=0, **kw)
    s4, d, _ = R.step(s3, c, 0.0, ROWS)
    assert d["applied"] and d["t"] == 2 and slot(st, 4) == R.state_words(s4)
    assert not torch.equal(o.p, data["p"])


def gn_sum_of(N, sizes, data, g, gn):
    return parent(N, sizes, data, g, 1, gn=gn).g2


def test_apply_skip_apply_counts_t_on_the_device(N, sizes, data):
    """Adam's t after a skipped pass is the device's applied count: the two applied calls of
    apply, skip, apply are the parent's with step = 1 and 2 (the second with the device's own
    1 - beta^t)."""
    g, kw = data["g_big"], dict(target_kl=TARGET, last_epoch=0, last_pass=0)
    gn = gn_partials(300, g)
    st = state_tensor(R.fresh_state(), 1)
    a, _ = ctl(N, sizes, data, g, st, 1, kl_table(8, 0.0), gn=gn, pass_index=0, **kw)
    assert a.same(parent(N, sizes, data, g, 1, gn=gn))
    nxt = {"p": a.p, "m1": a.m1, "m2": a.m2}
    b, _ = ctl(N, sizes, nxt, g, st, 2, kl_table(8, 64.0), gn=gn, pass_index=1, **kw)
    assert torch.equal(b.p, a.p) and torch.equal(b.m1, a.m1) and torch.equal(b.m2, a.m2)
    nxt = {"p": b.p, "m1": b.m1, "m2": b.m2}
    c3, _ = ctl(N, sizes, nxt, g, st, 3, kl_table(8, 0.0), gn=gn, pass_index=0, **kw)
    assert c3.same(parent(N, sizes, nxt, g, 2, gn=gn))
    words = slot(st, 3)
    assert (words[R.SLOTS.index("applied")], words[R.SLOTS.index("skipped")]) == (2, 1)


@pytest.mark.parametrize("scale", [1e-4, 0.5, 1.0 / 3.0, 1e3])
def test_effective_learning_rate_is_clamped(N, sizes, data, scale):
    """lr_nominal x scale below lr_min, inside, and above lr_max: the parent called with the
    clamped f64 product by value."""
    lr_min, lr_max = 1e-6, 1e-2
    want_lr = min(max(LR * scale, lr_min), lr_max)
    assert (scale == 1e-4) == (want_lr == lr_min) and (scale == 1e3) == (want_lr == lr_max)
    s = advanced(6)
    s["scale"] = scale
    g = data["g_small"]
    gn = gn_partials(64, g)
    row = torch.zeros(8, dtype=torch.float64, device="cuda")
    got, c = ctl(N, sizes, data, g, state_tensor(s, 7), 7, kl_table(4, 0.0), gn=gn, row=row, lr_min=lr_min, lr_max=lr_max)
    assert got.same(parent(N, sizes, data, g, 7, lr=want_lr, gn=gn))
    _, d, ref_row = R.step(s, c, 0.0, ROWS)
    assert d["lr"] == want_lr and [R.bits(x) for x in row.cpu().tolist()] == [R.bits(x) for x in ref_row]


# ------------------------------------------------------------------ a random sequence
def test_random_sequence_equals_the_restatement(N, sizes, data):
    """200 calls over several iterations, mixed flags, KLs on both sides of every threshold, the
    buffers swapped after every call as the trainer does: the state block and every emitted row
    equal the restatement bit for bit, and the master moves exactly on the applied passes."""
    rng = random.Random(99)
    lr_min, lr_max = 1e-5, 1e-3
    st = state_tensor(R.fresh_state(), 1)
    ref = R.fresh_state()
    cur = {k: data[k].clone() for k in ("p", "m1", "m2")}
    o = Out(sizes)
    g = data["g_small"]
    gn = gn_partials(300, g)
    row = torch.zeros(8, dtype=torch.float64, device="cuda")
    pass_index, rows_seen, decisions = 0, 0, []
    for call in range(1, 201):
        last_pass = int(rng.random() < 0.25)
        kw = dict(lr_nominal=rng.choice([3e-4, 1e-4, 2e-3, 4e-6]), lr_min=lr_min, lr_max=lr_max, target_kl=TARGET,
                  stop_factor=rng.choice([1.5, 1.5, math.inf]), adapt=rng.choice([0, 1, 1]),
                  adapt_factor=rng.choice([1.5, 2.0]), adapt_band=rng.choice([1.0, 2.0]), pass_index=pass_index,
                  last_epoch=int(last_pass or rng.random() < 0.5), last_pass=last_pass)
        rows = rng.choice([1024, 1280, 4096])
        # around the stop threshold (1.5 x), the band edges (0.5 x, 1 x, 2 x) and below zero
        kl_sum = rng.choice([-0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0]) * TARGET * rows + rng.randrange(-2, 3) * Q
        row.fill_(-1.0)
        _, c = ctl(N, sizes, cur, g, st, call, kl_table(rng.choice(COUNTS), kl_sum, seed=call), rows=rows, gn=gn,
                   out=o, row=row, **kw)
        ref, d, ref_row = R.step(ref, c, kl_sum, rows)
        assert slot(st, call) == R.state_words(ref), call
        assert torch.equal(o.p, cur["p"]) == (not d["applied"]), call
        if ref_row is None:
            assert row.cpu().tolist() == [-1.0] * 8, call  # only the iteration's last call writes it
        else:
            assert [R.bits(x) for x in row.cpu().tolist()] == [R.bits(x) for x in ref_row], call
            rows_seen += 1
        decisions.append(d["applied"])
        nxt = {"p": o.p, "m1": o.m1, "m2": o.m2}
        o.p, o.m1, o.m2 = cur["p"], cur["m1"], cur["m2"]
        cur = nxt
        pass_index = 0 if last_pass else pass_index + 1
    assert rows_seen > 20 and 20 < sum(decisions) < 180  # both branches were exercised
    assert ref["scale"] != 1.0
