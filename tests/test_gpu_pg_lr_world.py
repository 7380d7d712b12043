"""dxrl_pg_kl_rank_pack and dxrl_pg_adam_step_ctl_world on the device, through ctypes, with the
inputs and helpers of tests/test_gpu_pg_lr.py (random f32 master / gradient / moments of the real
parameter count).

The records are arbitrary doubles, so the merge order shows in the last bit: state words and rows
are compared bit for bit with tests/pg_lr_world_reference.py (the sequential rank-order merge, then
pg_lr_reference.step), and *_out, pack and gnorm2 with dxrl_pg_adam_step_ctl fed one loss block
whose column 3 holds the merged sum (0.0 + x == x) and the merged row count."""
import math
import random

import pytest
import torch

import pg_lr_reference as R
import pg_lr_world_reference as W
from test_gpu_pg_lr import (LR, BETAS, EPS, MAX_NORM, TARGET, N, Out, ctl, data, gn_partials, sizes, slot,  # noqa: F401
                            state_tensor)

pytestmark = pytest.mark.gpu

BLOCKS = (1, 3, 4, 5, 255, 256, 257)
WORLDS = (1, 2, 3, 8)


def pack(N, table, rows, record):
    N.call("dxrl_pg_kl_rank_pack", 0, N.ptr(table), table.shape[0], rows, N.ptr(record), None)
    torch.cuda.synchronize()
    return record.cpu().tolist()


def ctl_world(N, sizes, inp, g, state, calls, records, gn=None, out=None, row=None, **kw):
    """One dxrl_pg_adam_step_ctl_world call; records: f64 [world][2] on the device."""
    c = R.control(**dict(dict(lr_nominal=LR), **kw))
    k = N.PgLrControl(calls=calls, **c)
    o = out or Out(sizes)
    p = N.ptr
    scratch = torch.zeros(512, dtype=torch.float64, device="cuda") if gn is None else gn
    N.call("dxrl_pg_adam_step_ctl_world", 0, p(inp["p"]), p(g), p(inp["m1"]), p(inp["m2"]), p(o.p), p(o.m1), p(o.m2),
           sizes[0], BETAS[0], BETAS[1], EPS, MAX_NORM, p(scratch), 0 if gn is None else gn.numel(), p(o.g2),
           p(o.packed), p(records), records.shape[0], k, p(state), p(row), None)
    return o, c


def one_block(kl_sum):
    """A one-block loss table whose column-3 sum is kl_sum's bits."""
    t = torch.full((1, 4), 1e6, dtype=torch.float64)
    t[0, 3] = kl_sum
    return t.cuda()


def row_bits(row):
    return [R.bits(x) for x in row.cpu().tolist()]


# ------------------------------------------------------------------ the pack
@pytest.mark.parametrize("nb", BLOCKS)
def test_pack_is_the_fixed_order_sum_of_column_3(N, nb):
    """Random doubles of mixed magnitude in column 3 (any other order moves the last bits), NaN in
    columns 0-2 (a read of them poisons the sum)."""
    rng = random.Random(nb)
    col = [rng.uniform(-1.0, 1.0) * 10.0 ** rng.randrange(-6, 3) for _ in range(nb)]
    t = torch.full((nb, 4), float("nan"), dtype=torch.float64)
    t[:, 3] = torch.tensor(col, dtype=torch.float64)
    rows = 1280 + nb
    got = pack(N, t.cuda(), rows, torch.full((2,), -7.0, dtype=torch.float64, device="cuda"))
    assert R.bits(got[0]) == R.bits(W.column_sum(col)) and got[1] == float(rows), nb


def test_pack_refuses_bad_arguments_with_the_record_untouched(N):
    t = torch.ones(4, 4, dtype=torch.float64, device="cuda")
    rec = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    for table, nb, rows, record in ((None, 4, 128, rec), (t, 0, 128, rec), (t, -1, 128, rec), (t, 4, 0, rec),
                                    (t, 4, 128, None)):
        with pytest.raises(ValueError, match="kl_rank_pack"):
            N.call("dxrl_pg_kl_rank_pack", 0, N.ptr(table), nb, rows, N.ptr(record), None)
    torch.cuda.synchronize()
    assert rec.cpu().tolist() == [-7.0, -7.0]


# ------------------------------------------------------------------ the step
def records_for(rng, world, total_kl_sum):
    """world records with unequal rows whose KL sums are arbitrary doubles adding up to about
    total_kl_sum x (their rows / 1024): the global KL is about total_kl_sum / 1024."""
    rows = [512 + 256 * (r % 3) for r in range(world)]
    w = [rng.uniform(0.1, 1.0) for _ in range(world)]
    scale = total_kl_sum * sum(rows) / 1024.0 / sum(w)
    return [(x * scale, n) for x, n in zip(w, rows)]


# (pass_index, last_epoch, last_pass, KL sum per 1024 rows; the stop threshold is 12, the band 4 .. 16)
PLAN = ((0, 0, 0, 1.0), (1, 0, 0, 40.0), (2, 1, 1, 40.0),   # applied, stops at 1, copied through; adapts down
        (0, 0, 0, 1.0), (1, 1, 0, 2.0), (2, 1, 1, 2.0))     # three applied passes; adapts up


@pytest.mark.parametrize("clamps", [(1e-6, 1e-2), (2.5e-4, 3.5e-4)], ids=["wide", "tight"])
@pytest.mark.parametrize("world", WORLDS)
def test_six_passes_equal_the_restatement_and_the_one_rank_entry(N, sizes, data, world, clamps):
    """Two iterations of three passes through both state slots: an applied pass, the stop, a
    stopped copy-through with last_epoch / last_pass (scale / 1.5), then three applied passes (the
    first with the device's own 1 - beta^t) and scale x 1.5.  With the tight clamps lr x 2 / 3 is
    below lr_min and the next lr x 1.5 above lr_max, so the scale is moved to both bounds."""
    lr_min, lr_max = clamps
    rng = random.Random(1000 * world + int(lr_max * 1e6))
    g = data["g_small"]
    gn = gn_partials(300, g)
    st = state_tensor(R.fresh_state(), 1)
    ref = R.fresh_state()
    cur = {k: data[k].clone() for k in ("p", "m1", "m2")}
    scales = []
    for call, (u, le, lp, kl) in enumerate(PLAN, 1):
        recs = records_for(rng, world, kl)
        kw = dict(lr_min=lr_min, lr_max=lr_max, target_kl=TARGET, stop_factor=1.5, adapt=1, pass_index=u, last_epoch=le,
                  last_pass=lp)
        before = st.clone()
        row, row1 = (torch.full((8,), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
        o, c = ctl_world(N, sizes, cur, g, st, call, torch.tensor(recs, dtype=torch.float64).cuda(), gn=gn,
                         out=Out(sizes, sentinel=True), row=row, **kw)
        prev = ref
        ref, d, ref_row = W.step_world(ref, c, recs)
        assert slot(st, call) == R.state_words(ref), call
        assert st[(call - 1) & 1].cpu().tolist() == R.state_words(prev), call  # the slot read is left
        if ref_row is None:
            assert row.cpu().tolist() == [-1.0] * 8, call
        else:
            assert row_bits(row) == [R.bits(x) for x in ref_row], call
            scales.append(ref_row[R.COLUMNS.index("lr_scale")])
        # the one-rank entry from the same state, fed the merged pair
        kl_sum, rows = W.merge(recs)
        assert rows == int(rows)
        o1, _ = ctl(N, sizes, cur, g, before, call, one_block(kl_sum), rows=int(rows), gn=gn,
                    out=Out(sizes, sentinel=True), row=row1, **kw)
        assert o.same(o1) and torch.equal(before, st) and row_bits(row1) == row_bits(row), call
        assert torch.equal(o.p, cur["p"]) == (not d["applied"]), call
        if not d["applied"]:
            assert torch.equal(o.m1, cur["m1"]) and torch.equal(o.m2, cur["m2"])
            assert bool((o.packed.view(torch.int16) == 0x5A5A).all()), call
        cur = {"p": o.p, "m1": o.m1, "m2": o.m2}
    assert (ref["applied"], ref["skipped"], ref["stop_pass"]) == (4, 2, -1)
    if clamps == (2.5e-4, 3.5e-4):  # both clamps acted
        assert scales[0] in (lr_min / LR, math.nextafter(lr_min / LR, math.inf)) and LR * scales[0] >= lr_min
        assert scales[1] in (lr_max / LR, math.nextafter(lr_max / LR, 0.0)) and LR * scales[1] <= lr_max
    else:
        assert scales == [1.0 / 1.5, 1.0 / 1.5 * 1.5]


def test_the_global_kl_decides_on_the_device(N, sizes, data):
    """tests/test_pg_lr_world_host.py's two straddling cases: threshold 24 on 2 x 1024 rows."""
    g = data["g_small"]
    kw = dict(target_kl=TARGET, stop_factor=1.5, pass_index=1, last_epoch=0, last_pass=0)
    for recs, applied in (([(6.0, 1024), (20.0, 1024)], False), ([(20.0, 1024), (2.0, 1024)], True)):
        st = state_tensor(R.fresh_state(), 1)
        o, c = ctl_world(N, sizes, data, g, st, 1, torch.tensor(recs, dtype=torch.float64).cuda(), **kw)
        ref, d, _ = W.step_world(R.fresh_state(), c, recs)
        assert d["applied"] == applied and slot(st, 1) == R.state_words(ref)
        assert torch.equal(o.p, data["p"]) == (not applied)
        # rank 0's own record alone decides the other way
        alone = R.step(R.fresh_state(), c, *recs[0])[1]["applied"]
        assert alone != applied


@pytest.mark.parametrize("nb", [5, 257])
def test_world_one_with_a_packed_record_is_the_one_rank_entry(N, sizes, data, nb):
    """On the k_sumsq route (gnorm_blocks = 0), clip engaged: *_out, pack, gnorm2, state slot and
    row are dxrl_pg_adam_step_ctl's bytes when the record comes from the same partials."""
    rng = random.Random(nb)
    t = torch.full((nb, 4), 1e6, dtype=torch.float64)
    col = [rng.uniform(-1.0, 2.0) * 4.0 / nb for _ in range(nb)]  # a KL of about 2 / 1280: applied
    t[:, 3] = torch.tensor(col, dtype=torch.float64)
    t, rows, g = t.cuda(), 1280, data["g_big"]
    rec = torch.zeros(1, 2, dtype=torch.float64, device="cuda")
    pack(N, t, rows, rec)
    s = R.fresh_state()
    s.update(applied=6, skipped=1, scale=0.75)
    kw = dict(target_kl=TARGET, adapt=1, pass_index=3, last_epoch=1, last_pass=1)
    st_w, st_1 = state_tensor(s, 8), state_tensor(s, 8)
    row_w, row_1 = (torch.zeros(8, dtype=torch.float64, device="cuda") for _ in range(2))
    ow, _ = ctl_world(N, sizes, data, g, st_w, 8, rec, row=row_w, **kw)
    o1, _ = ctl(N, sizes, data, g, st_1, 8, t, rows=rows, row=row_1, **kw)
    torch.cuda.synchronize()
    assert ow.same(o1) and torch.equal(st_w, st_1) and row_bits(row_w) == row_bits(row_1)
    assert float(ow.g2) > MAX_NORM ** 2 and not torch.equal(ow.p, data["p"])
