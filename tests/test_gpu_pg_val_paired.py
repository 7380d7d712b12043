"""GPU: dxrl_pg_val_paired_row (csrc/dxrl_pg_val_paired.hip) on crafted level-major record
buffers, without an episode kernel, against the NumPy restatement
(tests/pg_val_paired_reference.py).

Shapes (L, G, K): one pair (NaN standard error); G K odd, so level 1 starts off 16-byte alignment
and takes the scalar loads; a mid-size case; 16 levels (every wave of the finish); and 66 chunks on
64 workgroups (the strided pass).  Kinds: random levels, every level a copy of the baseline,
returns near 1e6 with differences near 1e-3, every success lost, no discordant pair.

Bounds are test_gpu_pg_val_levels.py's: integer columns and object_lost exact; the three columns
derived from lost / gained equal to the restatement's f64 expression on the device's own
integers; mean_return_diff within sum_bound(d) / n; the two spreads within 1e-9 relative of the
two-pass f64 reduction.  Two calls on the same inputs give identical bytes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pg_val_paired_reference as P

pytestmark = pytest.mark.gpu

FILL, GUARD_I, PAD = 7.25, -7, 40


@pytest.fixture(scope="module")
def N():
    from dexterous_rl_manipulation_amd import _native
    _native.lib()
    return _native


class Harness:
    """Device copies of the records with PAD poisoned elements after each logical end (and
    `offset` before), the two tables with a guard row before and after, the scratch between NaN
    guards, the call."""

    def __init__(self, N, data, cap=4, offset=0):
        self.N, self.data, self.cap = N, data, cap
        dev = self.dev = torch.device("cuda:0")
        L, G, K = data["L"], data["G"], data["K"]

        def up(a, poison):
            a = np.asarray(a)
            full = np.concatenate([np.full(offset, poison, dtype=a.dtype), a.ravel(), np.full(PAD, poison, dtype=a.dtype)])
            return torch.from_numpy(full).to(dev)[offset:]

        self.t = {"ep_return": up(data["ep_return"], np.nan), "ep_length": up(data["ep_length"], 10 ** 6),
                  "ep_success": up(data["ep_success"], 255)}
        self.paired_all = torch.full((cap + 2, L, P.PAIRED_COLS), FILL, dtype=torch.float64, device=dev)
        self.paired = self.paired_all[1:cap + 1]
        self.lost_all = torch.full((cap + 2, L, G), GUARD_I, dtype=torch.int32, device=dev)
        self.lost = self.lost_all[1:cap + 1]
        nb = C.c_int64()
        N.call("dxrl_pg_val_paired_partial_doubles", L, G, K, C.byref(nb))
        self.partial_all = torch.full((nb.value + 2,), float("nan"), dtype=torch.float64, device=dev)
        self.partial = self.partial_all[1:nb.value + 1]

    def args(self, row, with_objects=True):
        N, d, p = self.N, self.data, self.N.ptr
        a = N.PgValPairedArgs()
        a.num_levels, a.num_objects, a.episodes_per_object, a.row, a.cap = d["L"], d["G"], d["K"], row, self.cap
        a.partial_doubles = self.partial.numel()
        for k in ("ep_return", "ep_length", "ep_success"):
            setattr(a, k, p(self.t[k]))
        a.partial, a.paired = p(self.partial), p(self.paired)
        if with_objects:
            a.object_lost = p(self.lost)
        return a

    def call(self, row, **kw):
        a = self.args(row, **kw)
        self.N.call("dxrl_pg_val_paired_row", 0, C.byref(a), self.N.stream_of(self.dev))
        torch.cuda.synchronize()
        return self.paired.cpu().numpy(), self.lost.cpu().numpy()

    def assert_guards(self, rows_written, object_rows=None):
        keep = [r for r in range(self.cap + 2) if r - 1 not in rows_written]
        assert np.all(self.paired_all.cpu().numpy()[keep] == FILL)
        keep = [r for r in range(self.cap + 2) if r - 1 not in (rows_written if object_rows is None else object_rows)]
        assert np.all(self.lost_all.cpu().numpy()[keep] == GUARD_I)
        p = self.partial_all.cpu().numpy()
        assert np.isnan(p[0]) and np.isnan(p[-1])

    def state_bytes(self):
        return tuple(x.cpu().numpy().tobytes() for x in (self.paired, self.lost))


def nan_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_rows(got_rows, got_lost, d):
    """One table row ([L][14]) and its per-object counts against the restatement, by the bounds of
    the module docstring."""
    L, G, K = d["L"], d["G"], d["K"]
    n = G * K
    rows, lost = P.paired_row(L, G, K, d["ep_return"], d["ep_length"], d["ep_success"])
    assert got_lost.tolist() == lost.tolist()
    for l in range(L):
        got = {name: got_rows[l, k] for k, name in enumerate(P.PAIRED_COLUMNS)}
        ref = rows[l]
        for name in P.INTEGER_COLUMNS + ("mean_length_diff",):
            assert got[name] == ref[name], (l, name)
        dev = P.derived(got["lost"], got["gained"], got["pairs"])  # on the device's own integers
        for name in P.DERIVED_COLUMNS:
            assert got[name] == dev[name] == ref[name], (l, name)
        ret0, ret1 = d["ep_return"][:n], d["ep_return"][l * n:(l + 1) * n]
        mean, std, stderr = P.two_pass(ret0, ret1)
        bound = P.sum_bound(ret1 - ret0) / n
        print("level", l, "mean_return_diff", got["mean_return_diff"], mean, bound, "std", got["return_diff_std"], std,
              "stderr", got["return_diff_stderr"], stderr)
        assert abs(got["mean_return_diff"] - mean) <= bound
        assert abs(got["mean_return_diff"] - ref["mean_return_diff"]) <= bound
        for have, want in ((got["return_diff_std"], std), (got["return_diff_stderr"], stderr)):
            if math.isnan(want):
                assert n == 1 and math.isnan(have)
            elif want == 0.0:
                assert have == 0.0
            else:
                assert abs(have - want) <= 1e-9 * want
    return rows


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("L,G,K", P.SHAPES)
def test_rows_against_the_restatement(N, L, G, K, kind):
    d = P.records(L, G, K, kind, seed=L + G + K)
    h = Harness(N, d)
    paired, lost = h.call(2)
    rows = check_rows(paired[2], lost[2], d)
    # level 0 is paired with itself: zeros, and NaN where n = 1 says so
    zero = np.zeros(P.PAIRED_COLS)
    zero[P.PIDX["pairs"]] = G * K
    s0 = int((d["ep_success"][:G * K] != 0).sum())
    zero[P.PIDX["both_success"]], zero[P.PIDX["both_fail"]] = s0, G * K - s0
    if G * K == 1:
        zero[P.PIDX["return_diff_stderr"]] = np.nan
    assert nan_equal(paired[2, 0], zero)
    if kind == "all_pairs_equal":
        assert all(nan_equal(paired[2, l], zero) for l in range(L)) and not lost[2].any()
    if kind == "every_success_lost":
        assert np.all(paired[2, 1:, P.PIDX["lost"]] == s0) and np.all(paired[2, 1:, P.PIDX["gained"]] == 0)
        assert np.all(paired[2, 1:, P.PIDX["paired_degradation"]] == s0 / (G * K))
    if kind == "no_discordant_pair":
        assert np.all(paired[2][:, [P.PIDX["lost"], P.PIDX["gained"], P.PIDX["mcnemar"]]] == 0.0)
    assert len(rows) == L
    h.assert_guards({2})


@pytest.mark.parametrize("L,G,K", [(2, 3, 5), (3, 37, 33), (2, 67, 1001)])
def test_repeat_calls_and_base_offsets_give_the_same_bytes(N, L, G, K):
    d = P.records(L, G, K, "random", seed=5)
    out = []
    for offset in (0, 0, 1, 3):
        h = Harness(N, d, offset=offset)
        h.call(1)
        first = h.state_bytes()
        h.call(1)  # again on the same harness: the scratch of the first call is in the way of nothing
        assert h.state_bytes() == first
        out.append(first)
        h.assert_guards({1})
    assert out[0] == out[1] == out[2] == out[3]


def test_a_null_object_table_leaves_the_paired_table_equal(N):
    d = P.records(3, 37, 33, "random", seed=1)
    h, h2 = Harness(N, d), Harness(N, d)
    paired, _ = h.call(0)
    paired2, _ = h2.call(0, with_objects=False)
    assert paired2[0].tobytes() == paired[0].tobytes()
    h.assert_guards({0})
    h2.assert_guards({0}, object_rows=set())


BAD = [
    ("num_levels", dict(num_levels=0)), ("num_levels", dict(num_levels=17)), ("num_levels", dict(num_levels=-1)),
    ("num_objects", dict(num_objects=0)), ("num_objects", dict(episodes_per_object=0)),
    ("INT32_MAX", dict(num_objects=1 << 16, episodes_per_object=1 << 15)),
    ("INT32_MAX", dict(num_levels=16, num_objects=1 << 14, episodes_per_object=1 << 14)),
    ("outside the table", dict(row=-1)), ("outside the table", dict(row=4)), ("outside the table", dict(cap=0)),
    ("null episode records", dict(ep_return=None)), ("null episode records", dict(ep_length=None)),
    ("null episode records", dict(ep_success=None)),
    ("null partial", dict(partial=None)), ("null partial", dict(paired=None)),
    ("partial holds", dict(partial_doubles=8)),
]


def test_invalid_arguments_return_before_any_launch_with_outputs_untouched(N):
    d = P.records(2, 3, 5, "random", seed=4)
    h = Harness(N, d)
    for match, change in BAD:
        a = h.args(0)
        for k, v in change.items():
            setattr(a, k, v)
        with pytest.raises(ValueError, match=match):
            N.call("dxrl_pg_val_paired_row", 0, C.byref(a), N.stream_of(h.dev))
    with pytest.raises(ValueError, match="null args"):
        N.call("dxrl_pg_val_paired_row", 0, None, N.stream_of(h.dev))
    torch.cuda.synchronize()
    h.assert_guards(set())
    assert np.isnan(h.partial_all.cpu().numpy()).all()  # not even the scratch was written
