"""GPU: dxrl_pg_log_rank_pack and dxrl_pg_log_row_world (csrc/dxrl_pg_log.hip) on uploaded arrays,
without a trainer or a process group: the "all-gather" is a device copy of every rank's record
into records[world][DXRL_PG_LOG_RANK_DOUBLES].  Buffers are those of tests/test_gpu_pg_log.py's
Harness (NaN-poisoned padding past every logical end, a huge sentinel in the bootstrap slot of
values, a FILL-ed table, NaN-filled partial), with NaN-filled record / records and a FILL-ed
rank_log beside them.

Bounds: tests/test_gpu_pg_log.py's (pg_log_world_reference.assert_row_within_bounds)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pg_log_reference as L
import pg_log_world_reference as W
from test_gpu_pg_log import FILL, SHAPES, Harness

pytestmark = pytest.mark.gpu

R = W.RANK_DOUBLES
T = 33
NUM_PARAMS = 1031
STATS = np.arange(8) * 0.375 - 1.0   # the caller's (global) advantage statistics
GNORM2 = 2.75
# ragged shards: 33, 528 and 4,290 samples are one partial group, one workgroup, two workgroups + tail
SIZES = {2: (16, 130), 3: (1, 16, 130), 5: (130, 1, 16, 1, 130)}
EMPTY_RANK = 1                       # the rank that finished no episode


@pytest.fixture(scope="module")
def N():
    from dexterous_rl_manipulation_amd import _native
    _native.lib()
    return _native


def stream():
    return torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream


def nan_doubles(count, offset):
    """`count` NaN doubles on the device, `offset` elements into their allocation."""
    return torch.full((count + offset,), float("nan"), dtype=torch.float64, device="cuda:0")[offset:]


class Rank(Harness):
    """One rank's buffers and its record."""

    def __init__(self, N, data, offset=0, **kw):
        super().__init__(N, dict(data, stats=STATS, gnorm2=GNORM2), offset=offset, **kw)
        self.record = nan_doubles(R, offset)

    def pack(self, **kw):
        a = self.args(kw.pop("row", 0), **kw)
        self.N.call("dxrl_pg_log_rank_pack", 0, C.byref(a), self.N.ptr(self.record), stream())
        return self.record


class World:
    """The ranks of one sharded iteration.  Rank 0's harness holds the table, header and best
    parameters the row is finished into; `records` and `rank_log` stand beside them."""

    def __init__(self, N, shards, cap=4, pad="nan", offset=0, num_params=0):
        self.N, self.world, self.cap = N, len(shards), cap
        self.ranks = [Rank(N, d, offset=offset, cap=cap, pad=pad, num_params=num_params if r == 0 else 0)
                      for r, d in enumerate(shards)]
        self.head = self.ranks[0]
        self.records = nan_doubles(self.world * R, offset)
        self.rank_log = torch.full((cap * self.world * R + offset,), FILL, dtype=torch.float64, device="cuda:0")[offset:]

    def gather(self, **kw):
        for r, rank in enumerate(self.ranks):
            self.records[r * R:(r + 1) * R].copy_(rank.pack(**kw))

    def finish(self, row, rank_log=True, **kw):
        a = self.head.args(row, **kw)
        p = self.N.ptr
        self.N.call("dxrl_pg_log_row_world", 0, C.byref(a), p(self.records), self.world,
                    p(self.rank_log) if rank_log else None, stream())
        torch.cuda.synchronize()
        return self.head.table.cpu().numpy()

    def call(self, row, **kw):
        self.gather(row=row, **kw)
        return self.finish(row, **kw)

    def state(self):
        """Every byte the pair may write."""
        h = self.head
        torch.cuda.synchronize()
        out = [h.table.cpu().numpy().tobytes(), h.header.cpu().numpy().tobytes(),
               self.records.cpu().numpy().tobytes(), self.rank_log.cpu().numpy().tobytes()]
        if h.best is not None:
            out.append(h.best.cpu().numpy().tobytes())
        return out


def one_rank(n, T, seed):
    return W.shard_inputs(n, T, seed)


# ------------------------------------------------------------------ 1. world 1 == dxrl_pg_log_row
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n,T", SHAPES)
def test_world_one_writes_the_bytes_of_log_row(N, n, T, offset):
    """pack + row_world on the single record against dxrl_pg_log_row on the same inputs, over a
    scripted series of 4 rows with a tie (row 2) and a NaN score (row 3), keep-best (1031
    parameters) and convergence on: table, header and best_params byte-equal after every row."""
    d = one_rank(n, T, seed=n)
    scores, episodes = [1.0, 3.0, 3.0, float("nan")], [4, 4, 4, 4]
    want_rows, _, _ = L.series_rules(scores, episodes, 2, [0.0] * 4, 1, 1e9)
    assert want_rows == [0, 1]
    rules = dict(score_col=L.IDX["mean_return"], min_episodes=2, conv_col=L.IDX["mean_step_reward"], window=2,
                 threshold=-1e9)
    one = Harness(N, dict(d, stats=STATS, gnorm2=GNORM2), offset=offset, num_params=NUM_PARAMS)
    wld = World(N, [d], offset=offset, num_params=NUM_PARAMS)
    if offset:
        assert all(h.t[k].data_ptr() % 16 for h in (one, wld.head) for k in ("rew", "ret", "done", "values"))
        assert wld.records.data_ptr() % 16 and wld.head.record.data_ptr() % 16 and wld.rank_log.data_ptr() % 16
    for r in range(4):
        cnt, ret = np.zeros(n, dtype=np.int32), np.zeros(n)
        cnt[3], ret[3] = episodes[r], scores[r] * episodes[r]
        for h in (one, wld.head):
            h.t["ep_count"][:n].copy_(torch.from_numpy(cnt))
            h.t["ep_sum_return"][:n].copy_(torch.from_numpy(ret))
            h.t["rew"][:n * T].mul_(0.5).add_(float(r))  # another mean_step_reward per row, the same on both
            h.params.copy_(1000.0 * (r + 1) + torch.arange(NUM_PARAMS, device="cuda:0"))
        ta = one.call(r, iteration=10 + r, env_steps=(r + 1) * n * T, **rules)
        tb = wld.call(r, iteration=10 + r, env_steps=(r + 1) * n * T, **rules)
        assert ta[r, L.IS_BEST] == float(r in want_rows), r
        assert tb.tobytes() == ta.tobytes(), r
        assert wld.head.header.cpu().numpy().tobytes() == one.header.cpu().numpy().tobytes(), r
        assert torch.equal(wld.head.best, one.best), r
        rank_log = wld.rank_log.cpu().numpy().reshape(wld.cap, R)
        assert rank_log[r].tobytes() == wld.records.cpu().numpy().tobytes() and np.all(rank_log[r + 1:] == FILL), r
    assert one.head()["best_row"] == 1 and one.head()["converged_row"] == 1 and one.head()["rows_written"] == 4
    assert math.isnan(ta[3, L.IDX["mean_return"]])


# ------------------------------------------------------------------ 2. / 3. world W
def world_shards(world):
    return [W.shard_inputs(n, T, seed=100 * world + r, episodes=r != EMPTY_RANK) for r, n in enumerate(SIZES[world])]


@pytest.mark.parametrize("world", sorted(SIZES))
def test_world_row_against_the_restatement(N, world):
    shards = world_shards(world)
    wld = World(N, shards)
    row, rules = 2, dict(score_col=L.IDX["mean_return"], conv_col=L.IDX["episodes"], window=1, threshold=0.0)
    table = wld.call(row, iteration=3, env_steps=1234567, **rules)
    got = {name: table[row, k] for k, name in enumerate(L.COLUMNS)}
    c = W.concatenated(shards)
    ref = L.row_values(c["n"], T, 3, 1234567, c["ep_count"], c["ep_sum_return"], c["ep_sum_length"], c["ep_successes"],
                       c["rew"], c["ret"], c["done"], c["values"], STATS, c["loss_partial"], c["loss_rows"], GNORM2)
    W.assert_row_within_bounds(got, ref, c["ep_sum_return"], c["rew"], c["ret"], c["values"], c["loss_partial"],
                               c["loss_rows"], what=f"world {world}")
    # keep-best and the window rule, restated on the reference's values
    want_table, want_header = np.full((wld.cap, L.COLS), FILL), L.new_header()
    assert L.finish_row(want_table, want_header, row, ref, L.IDX["mean_return"], 1, L.IDX["episodes"], 1, 0.0)
    assert got["is_best"] == 1.0 and got["window_mean"] == ref["episodes"] == want_table[row, L.IDX["window_mean"]]
    head = wld.head.head()
    assert head == dict(want_header, best_score=got["mean_return"])
    assert np.all(table[row, len(L.COLUMNS):] == 0.0) and np.all(table[[0, 1, 3]] == FILL)
    # the record of every rank, against its restatement
    recs = wld.records.cpu().numpy().reshape(world, R)
    for r, d in enumerate(shards):
        want = W.record_of(d)
        for name in ("samples", "done_count", "episodes", "length_sum", "successes", "loss_rows"):
            assert recs[r, W.R[name]] == want[W.R[name]], (r, name)
        assert np.all(recs[r, len(W.RANK_COLUMNS):] == 0.0)
        M = d["n"] * T
        for name, terms in (("reward_sum", d["rew"]), ("value_sum", d["values"][:M]), ("return_sum", d["ep_sum_return"])):
            assert abs(recs[r, W.R[name]] - want[W.R[name]]) <= W.sum_bound(terms), (r, name)
        for name in ("target_m2", "residual_m2"):
            assert abs(recs[r, W.R[name]] - want[W.R[name]]) <= 1e-9 * want[W.R[name]], (r, name)
    assert recs[EMPTY_RANK, W.R["episodes"]] == 0.0
    # rank_log: row `row` holds the gathered records byte for byte, the other rows keep FILL
    log = wld.rank_log.cpu().numpy().reshape(wld.cap, world, R)
    assert log[row].tobytes() == recs.tobytes() and np.all(log[[0, 1, 3]] == FILL)


@pytest.mark.parametrize("world", [3])
def test_world_row_is_deterministic_and_reads_nothing_past_an_end(N, world):
    shards = world_shards(world)
    rules = dict(score_col=L.IDX["mean_return"], conv_col=L.IDX["mean_return"], window=1, threshold=0.0)
    wld = World(N, shards, num_params=NUM_PARAMS)
    wld.head.params.fill_(4.0)
    wld.call(2, **rules)
    first = wld.state()
    assert torch.all(wld.head.best == 4.0)
    # a second call on the same buffers (header as the first call left it: the same row, no new best)
    fresh = World(N, shards, num_params=NUM_PARAMS)
    fresh.head.params.fill_(4.0)
    fresh.call(2, **rules)
    assert fresh.state() == first
    wld.gather(row=2, **rules)
    again = wld.finish(2, **rules)
    assert again[2, :L.IS_BEST].tobytes() == np.frombuffer(first[0], dtype=np.float64).reshape(-1, L.COLS)[2, :L.IS_BEST].tobytes()
    assert wld.records.cpu().numpy().tobytes() == first[2] and wld.rank_log.cpu().numpy().tobytes() == first[3]
    # zero padding and a clean bootstrap slot instead of NaN poison: identical bytes
    clean = World(N, shards, pad="zero", num_params=NUM_PARAMS)
    clean.head.params.fill_(4.0)
    clean.call(2, **rules)
    assert clean.state() == first
    # one element off 16-byte alignment: the same bytes
    off = World(N, shards, offset=1, num_params=NUM_PARAMS)
    off.head.params.fill_(4.0)
    off.call(2, **rules)
    assert off.state() == first
    # rank_log is optional
    bare = World(N, shards, num_params=NUM_PARAMS)
    bare.head.params.fill_(4.0)
    bare.gather(row=2, **rules)
    bare.finish(2, rank_log=False, **rules)
    assert bare.state()[:3] == first[:3] and torch.all(bare.rank_log == FILL)


# ------------------------------------------------------------------ 4. no episodes anywhere
def test_zero_episodes_on_every_rank_give_nan_and_are_never_best(N):
    shards = [W.shard_inputs(n, T, seed=7 + r, episodes=False) for r, n in enumerate((16, 1, 130))]
    wld = World(N, shards, num_params=8)
    row = wld.call(0, score_col=L.IDX["mean_return"], min_episodes=0, conv_col=L.IDX["mean_return"], window=1)[0]
    g = {name: row[k] for k, name in enumerate(L.COLUMNS)}
    assert g["episodes"] == 0.0
    assert all(math.isnan(g[k]) for k in ("mean_return", "mean_length", "success_rate"))
    assert g["is_best"] == 0.0 and math.isnan(g["window_mean"])
    assert math.isfinite(g["target_var"]) and g["target_var"] > 0.0
    assert wld.head.head() == dict(L.new_header(), rows_written=1)
    assert torch.all(wld.head.best == -1.0)


# ------------------------------------------------------------------ 5. argument errors
def test_argument_errors_write_nothing(N):
    shards = [W.shard_inputs(16, 2, seed=r) for r in range(2)]
    wld = World(N, shards, num_params=8)
    h, p = wld.head, N.ptr
    rules = dict(score_col=L.IDX["mean_return"], conv_col=L.IDX["mean_return"], window=2)
    pack = lambda a, rec: N.call("dxrl_pg_log_rank_pack", 0, a, rec, stream())  # noqa: E731
    row_world = lambda a, recs, world, log: N.call("dxrl_pg_log_row_world", 0, a, recs, world, log, stream())  # noqa: E731
    a = h.args(1, **rules)
    for fn, msg in ((lambda: pack(None, p(h.record)), "null args"), (lambda: pack(C.byref(a), None), "null record"),
                    (lambda: row_world(None, p(wld.records), 2, p(wld.rank_log)), "null args"),
                    (lambda: row_world(C.byref(a), None, 2, p(wld.rank_log)), "null records"),
                    (lambda: row_world(C.byref(a), p(wld.records), 0, p(wld.rank_log)), "world"),
                    (lambda: row_world(C.byref(a), p(wld.records), -3, p(wld.rank_log)), "world")):
        with pytest.raises(ValueError, match=msg):
            fn()
    # everything dxrl_pg_log_row refuses (tests/test_gpu_pg_log.py's cases), on both entries
    cases = [("row", 4, "outside the table"), ("row", -1, "outside the table"), ("cap", 0, "outside the table"),
             ("num_envs", 0, "num_envs"), ("horizon", 0, "horizon"),
             ("score_col", L.IS_BEST, "score_col"), ("score_col", L.COLS, "score_col"),
             ("conv_col", L.IS_BEST, "conv_col"), ("conv_col", 99, "conv_col"), ("conv_window", 0, "conv_window"),
             ("loss_rows", 0, "loss_rows"), ("loss_blocks", -1, "loss_blocks"), ("partial_doubles", 1, "partial holds"),
             ("best_params", None, "keep-best"), ("num_params", 0, "keep-best")]
    cases += [(k, None, "null") for k in ("ep_count", "ep_sum_return", "ep_sum_length", "ep_successes", "rew", "ret",
                                          "done", "values", "stats", "loss_partial", "gnorm2", "partial", "log",
                                          "header")]
    for field, value, msg in cases:
        a = h.args(1, **rules)
        setattr(a, field, value)
        with pytest.raises(ValueError, match=msg):
            pack(C.byref(a), p(h.record))
        with pytest.raises(ValueError, match=msg):
            row_world(C.byref(a), p(wld.records), 2, p(wld.rank_log))
    torch.cuda.synchronize()
    assert torch.all(h.table == FILL) and torch.all(h.best == -1.0) and torch.all(wld.rank_log == FILL)
    assert h.head() == L.new_header()
    assert torch.isnan(h.record).all() and torch.isnan(wld.records).all() and torch.isnan(h.partial).all()
