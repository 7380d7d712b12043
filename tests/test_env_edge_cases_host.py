"""CPU: the crafted edge lanes (tests/env_edge_cases.py) do what their names say.

The GPU tests in test_gpu_env_edges.py compare the device's env-step implementations with the
oracle on these lanes; they prove nothing if a lane misses its edge.  Here the oracle runs over
every lane and ``check`` asserts, from the oracle's own state, that each lane meets its named edge
at its named step, that every cell of every family is present, and that no episode ends early."""
import math

import numpy as np
import pytest

import env_edge_cases as E


@pytest.fixture(scope="module", params=["state", "reset"])
def cases(request):
    return E.build(request.param)


def test_every_lane_meets_its_named_edge(cases):
    traces = E.check(cases)
    L = len(cases)
    assert len(traces) == L and L % 16 and L % 32 and L % 256
    if cases.mode == "state":
        assert 1200 < L < 1500
    assert cases.actions().shape == (E.T, L, E.D)


@pytest.mark.parametrize("family", E.FAMILIES)
def test_checker_notices_a_missing_family(family):
    for mode in ("state", "reset"):
        if family == "trunc" and mode == "reset":
            continue  # a reset starts at step count 0: the family has no reset lanes
        part = E.build(mode, families=[f for f in E.FAMILIES if f != family])
        with pytest.raises(AssertionError, match="cells missing"):
            E.check(part)


def test_checker_notices_a_lane_off_its_edge():
    """A knife-edge lane moved 2^-30 relative off its size, a wall lane pulled off its wall and a joint
    lane that no longer reaches its bound each fail the check."""
    for family, cell, spoil in (
            ("knife", ("post0", 0, 0), lambda ln: setattr(ln, "size", ln.size * (1 + 2.0 ** -30))),
            ("wall", (0, "lo", "into", "on", 1, 0), lambda ln: ln.op.__setitem__(0, 0.0)),
            ("joint", (0, 1, "cross"), lambda ln: ln.jp.__setitem__(0, 0.0))):
        cases = E.build("state")
        lane = next(ln for ln in cases.lanes if (ln.family, ln.cell) == (family, cell))
        spoil(lane)
        with pytest.raises(AssertionError, match=family):
            E.check(cases)


def test_knife_edge_sizes_sit_in_the_slow_path_band(cases):
    """The knife-edge lanes' squared distance is within 2^-40 relative of the squared threshold
    (csrc/dxrl_device.h sqrt_below takes the exact root only there), and the oracle's contact bit
    follows d < 1.5 size on each of them."""
    n = 0
    for i, ln in enumerate(cases.lanes):
        if ln.family != "knife" or len(ln.cell) != 3:
            continue
        s = E.trace(cases, i)[ln.step]
        f = ln.cell[1]
        assert abs(s["dist"][f] - s["thr"]) <= 4 * math.ulp(s["thr"]), ln.name
        assert ((s["mask"] >> f) & 1) == int(s["dist"][f] < s["thr"])
        n += 1
    assert n == 5 * 5 * (2 if cases.mode == "state" else 3)


def test_flags_and_draws_round_trip(cases):
    """The slab words and reset draws the GPU tests write restate the lanes."""
    fl = cases.flags()
    for i, ln in enumerate(cases.lanes):
        assert bool(fl[i] & E.OP_IS_F32) == ln.op_is_f32 and bool(fl[i] & E.FRIC_F64) == ln.fric_f64
        assert bool(fl[i] & E.HAS_PREV) == (ln.prev is not None)
        if ln.prev is not None:
            assert (fl[i] >> E.PREV_SHIFT) & 0xFF == ln.prev
        if ln.op_is_f32:
            assert np.array_equal(ln.op, ln.op.astype(np.float32).astype(np.float64)), ln.name
    if cases.mode == "reset":
        d = cases.reset_draws()
        assert d.shape == (len(cases), 21) and not np.isnan(d).any()
        for ln in cases.lanes:
            assert ln.t == 0 and ln.prev is None and not ln.jv.any() and not ln.ov.any() and ln.op_is_f32
