"""GPU checks of dxrl_study_summarize on uploaded records (tests/study_summary_cases.py) against
its NumPy restatement (tests/study_summary_reference.py): integers, tie list and status equal, f64
columns bit for bit (same operations in the same order), repeatable bytes, lane_offset, every
status bit provoked with in-range memory, argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from dexterous_rl_manipulation_amd import _native as N
from dexterous_rl_manipulation_amd import curriculum_ablation as CA

import study_summary_cases as K
import study_summary_reference as S
from test_study_summary_host import csr, groups_of

pytestmark = pytest.mark.gpu

W, THR = K.W, K.THR
C_MIN = CA.min_successes(W, 0.5)


class Tables:
    def __init__(self, L, G, tie_cap, dev):
        self.lane_ints = torch.zeros(L, 8, dtype=torch.int64, device=dev)
        self.lane_reals = torch.zeros(L, 4, dtype=torch.float64, device=dev)
        self.group_stats = torch.full((max(G, 1), 16), -5, dtype=torch.int64, device=dev)
        self.group_metrics = torch.full((max(G, 1), 5, 3), -5.0, dtype=torch.float64, device=dev)
        self.tie_count = torch.full((1,), -5, dtype=torch.int32, device=dev)
        self.tie_list = torch.full((max(tie_cap, 1),), -5, dtype=torch.int32, device=dev)
        self.status = torch.full((1,), -5, dtype=torch.int32, device=dev)  # the call zeroes it

    def host(self):
        return [t.cpu().numpy() for t in (self.lane_ints, self.lane_reals, self.group_stats, self.group_metrics,
                                          self.tie_count, self.tie_list, self.status)]


def summarize(case, groups=None, tie_cap=None, episodes=None, parts=None, offsets=None, flat=None, num_members=None,
              window=W, record_cap=None, null=()):
    """Upload ``case`` (in ``parts`` = [(lo, hi), ...] separate buffers when given) and call the
    entry point once per buffer; returns the host copies of every output."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(case["episodes"])
    eps = case["episodes"] if episodes is None else np.asarray(episodes, dtype=np.int32)
    if groups is not None:
        offsets, flat, _ = csr(groups)
    G = 0 if offsets is None else len(offsets) - 1
    tie_cap = n if tie_cap is None else tie_cap
    t = Tables(n, G, tie_cap, dev)
    keep = []
    parts = parts or [(0, n)]
    statuses = []
    for k, (lo, hi) in enumerate(parts):
        up = {key: torch.from_numpy(np.ascontiguousarray(case[key][lo:hi])).to(dev)
              for key in ("ep_return", "ep_length", "ep_success")}
        lvl = None if case["ep_level"] is None else torch.from_numpy(np.ascontiguousarray(case["ep_level"][lo:hi])).to(dev)
        ne = torch.from_numpy(np.ascontiguousarray(eps[lo:hi])).to(dev)
        keep += [up, lvl, ne]
        a = N.StudySummaryArgs()
        a.num_lanes, a.record_cap, a.lane_offset, a.total_lanes = hi - lo, record_cap or case["cap"], lo, n
        a.window, a.min_count, a.reward_threshold = window, C_MIN, THR
        a.ep_return, a.ep_length, a.ep_success = (N.ptr(up[key]) for key in ("ep_return", "ep_length", "ep_success"))
        a.ep_level, a.lane_episodes = N.ptr(lvl), N.ptr(ne)
        a.lane_ints, a.lane_reals, a.status = N.ptr(t.lane_ints), N.ptr(t.lane_reals), N.ptr(t.status)
        if k == len(parts) - 1 and offsets is not None:
            go = torch.from_numpy(np.asarray(offsets, dtype=np.int32)).to(dev)
            gl = torch.from_numpy(np.asarray(flat, dtype=np.int32)).to(dev)
            keep += [go, gl]
            a.num_groups, a.num_members, a.tie_cap = G, len(flat) if num_members is None else num_members, tie_cap
            a.group_offsets, a.group_lanes = N.ptr(go), N.ptr(gl)
            a.group_stats, a.group_metrics = N.ptr(t.group_stats), N.ptr(t.group_metrics)
            a.tie_count, a.tie_list = N.ptr(t.tie_count), N.ptr(t.tie_list)
        for name in null:
            setattr(a, name, None)
        N.call("dxrl_study_summarize", dev.index, C.byref(a), N.stream_of(dev))
        statuses.append(int(t.status.item()))
    return t.host(), statuses


def expected(case, groups=None, tie_cap=None, episodes=None, offsets=None, flat=None, num_members=None):
    eps = case["episodes"] if episodes is None else episodes
    ints, reals, st = S.lane_pass(case["ep_return"], case["ep_length"], case["ep_success"], case["ep_level"], eps, W,
                                  C_MIN, THR)
    if groups is not None:
        offsets, flat, _ = csr(groups)
    if offsets is None:
        return ints, reals, st
    stats, metrics, ties, count, gst = S.group_pass(ints, reals, offsets, flat,
                                                    len(ints) if tie_cap is None else tie_cap, num_members)
    return ints, reals, stats, metrics, ties, count, st | gst


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("case", [K.random_ragged, K.random_uniform, K.crafted])
def test_summary_equals_restatement_bit_for_bit(case):
    c, groups = case(), groups_of(case)
    (ints, reals, stats, metrics, tcount, tlist, status), _ = summarize(c, groups)
    wi, wr, ws, wm, wt, wc, wst = expected(c, groups)
    assert np.array_equal(ints, wi)
    assert same_bits(reals, wr)
    assert np.array_equal(stats, ws)
    assert same_bits(metrics, wm)
    assert int(tcount[0]) == wc and tlist[:wc].tolist() == wt and int(status[0]) == wst
    assert wc == (1 if case is K.crafted else 0)
    again, _ = summarize(c, groups)
    for a, b in zip((ints, reals, stats, metrics, tcount, tlist, status), again):
        assert a.tobytes() == b.tobytes()


def test_two_buffers_with_lane_offset_equal_one_buffer():
    c, groups = K.random_ragged(), groups_of(K.random_ragged)
    one, _ = summarize(c, groups)
    two, statuses = summarize(c, groups, parts=[(0, 6), (6, 16)])
    assert statuses == [0, S.ST_MIXED]
    for a, b in zip(one, two):
        assert a.tobytes() == b.tobytes()


def test_long_rows_are_read_without_staging():
    """record_cap above the LDS staging bound takes the kernel's other path: same tables."""
    c = K.random_uniform()
    cap = 8200
    big = dict(c, cap=cap)
    for key, fill in (("ep_return", np.nan), ("ep_length", -7), ("ep_success", 1)):
        buf = np.full((12, cap), fill, dtype=c[key].dtype)
        buf[:, :c["cap"]] = c[key]
        big[key] = buf
    groups = groups_of(K.random_uniform)
    got, _ = summarize(big, groups)
    want, _ = summarize(c, groups)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()


def test_status_bits():
    c = K.random_uniform()
    n = 12
    # bit 0: a group offset past the member list, a member past the lane table (in-range memory only)
    for offsets, flat, members in (([0, 4, 9], [0, 1, 2, 3, 4, 5, 6, 7], 8), ([0, 3], [0, 12, 1], 3),
                                   ([0, 2, 1], [0, 1, 2], 3)):
        got, _ = summarize(c, offsets=offsets, flat=flat, num_members=members)
        want = expected(c, offsets=offsets, flat=flat, num_members=members)
        assert int(got[6][0]) == want[6] and want[6] & S.ST_RANGE
        assert np.array_equal(got[2], want[2]) and same_bits(got[3], want[3])
    # bit 1: tie_cap = 0 (the count stays true, the list untouched)
    cr = K.crafted()
    got, _ = summarize(cr, {"all": list(range(len(K.CRAFTED)))}, tie_cap=0)
    assert int(got[6][0]) == S.ST_TIE_CAP | S.ST_MIXED and int(got[4][0]) == 1 and got[5].tolist() == [-5]
    # bit 2: E = 0 and E > record_cap: those lanes are skipped
    eps = c["episodes"].copy()
    eps[3], eps[5] = 0, c["cap"] + 1
    groups = {"a": [0, 1, 2, 3], "b": [4, 5, 6, 7]}
    got, _ = summarize(c, groups, episodes=eps)
    want = expected(c, groups, episodes=eps)
    assert int(got[6][0]) == want[6] == S.ST_LANE
    assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and same_bits(got[3], want[3])
    assert got[2][0, 0] == 3 and got[2][1, 0] == 3
    # bit 3: mixed E in a group
    eps = c["episodes"].copy()
    eps[1] = 33
    got, _ = summarize(c, groups, episodes=eps)
    want = expected(c, groups, episodes=eps)
    assert int(got[6][0]) == want[6] == S.ST_MIXED and np.array_equal(got[2], want[2])
    assert n == len(eps)


def test_argument_errors():
    c = K.random_uniform()
    for kw in ({"window": 0}, {"window": 65}, {"record_cap": -1}, {"null": ("ep_return",)}, {"null": ("lane_ints",)},
               {"null": ("status",)}, {"null": ("lane_episodes",)}):
        with pytest.raises(ValueError):
            summarize(c, **kw)
    with pytest.raises(ValueError, match="group_metrics"):
        summarize(c, groups_of(K.random_uniform), null=("group_metrics",))
