"""GPU: dxrl_pg_val_levels_row (csrc/dxrl_pg_val_levels.hip) on crafted level-major record
buffers, without an episode kernel, against the NumPy restatement
(tests/pg_val_levels_reference.py) and against dxrl_pg_val_row on every level's slice.

Shapes (L, G, K): the smallest launch; ragged against the wave, the 4 records of a thread and the
1,024 of a workgroup; the 16-level and 256-object bounds together; G K odd, so levels 1 and 2
start off 16-byte alignment and take the scalar loads while level 0 takes the vector loads; and
more than 65,536 records per level (the grid-stride loop).

Bounds are test_gpu_pg_val.py's: integers, rates and flags exact; mean_return within
sum_bound / count of the level's returns; return_std within 1e-9 relative of the two-pass value.
The degradation and robust columns are formed from exact rates by the restatement's own f64
operations, so they are compared with ==.  A level's eight statistic columns and its object
counts are the bytes dxrl_pg_val_row writes for that slice."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pg_val_levels_reference as R
import pg_val_reference as V
import test_gpu_pg_val as T

pytestmark = pytest.mark.gpu

FILL, GUARD_I, GUARD_P, PAD, NP = T.FILL, T.GUARD_I, T.GUARD_P, T.PAD, T.NP
SHAPES = [(1, 1, 1), (2, 3, 5), (5, 7, 7), (16, 256, 1), (3, 37, 33), (2, 67, 1001)]
KINDS = T.KINDS + ["baseline_all_fail", "one_level_all_fail"]
WORST_RETURN = R.RIDX["worst_mean_return"]


@pytest.fixture(scope="module")
def N():
    from dexterous_rl_manipulation_amd import _native
    _native.lib()
    return _native


def level_records(L, G, K, kind="random", seed=0):
    """Level-major records: T.records of `kind` per level (its own seed); the two extra kinds are
    random levels with the baseline, or the last level, all failing."""
    per = [T.records(G, K, kind if kind in T.KINDS else "random", seed=seed + 17 * l) for l in range(L)]
    d = {k: np.concatenate([p[k] for p in per]) for k in ("ep_return", "ep_length", "ep_success", "ep_contacts")}
    if kind == "baseline_all_fail":
        d["ep_success"][:G * K] = 0
    elif kind == "one_level_all_fail":
        d["ep_success"][(L - 1) * G * K:] = 0
    d.update(L=L, G=G, K=K, status=per[0]["status"],
             noise=[(0.0, 0.0)] + [(0.01 * l, 0.5 / l) for l in range(1, L)])
    return d


class Harness:
    """Device copies of `level_records` with PAD poisoned elements after each logical end (and
    `offset` before), the three tables and the object counts with a guard row before and after,
    best_params with guard words, the scratch between NaN guards, a fresh header, the call."""

    def __init__(self, N, data, cap=4, offset=0, params_offset=1):
        self.N, self.data, self.cap = N, data, cap
        dev = self.dev = torch.device("cuda:0")
        L, G, K = data["L"], data["G"], data["K"]

        def up(a, poison):
            a = np.asarray(a)
            full = np.concatenate([np.full(offset, poison, dtype=a.dtype), a.ravel(), np.full(PAD, poison, dtype=a.dtype)])
            return torch.from_numpy(full).to(dev)[offset:]

        self.t = {"ep_return": up(data["ep_return"], np.nan), "ep_length": up(data["ep_length"], 10 ** 6),
                  "ep_success": up(data["ep_success"], 255), "ep_contacts": up(data["ep_contacts"], 255)}
        self.status = torch.tensor([data["status"]], dtype=torch.int32, device=dev)
        self.noise = torch.tensor(data["noise"], dtype=torch.float64, device=dev)
        full = lambda *shape: torch.full(shape, FILL, dtype=torch.float64, device=dev)  # noqa: E731
        self.table_all, self.levels_all, self.robust_all = full(cap + 2, V.COLS), full(cap + 2, L, R.LEVEL_COLS), \
            full(cap + 2, R.ROBUST_COLS)
        self.table, self.levels, self.robust = (x[1:cap + 1] for x in (self.table_all, self.levels_all, self.robust_all))
        self.objects_all = torch.full((cap + 2, L, G), GUARD_I, dtype=torch.int32, device=dev)
        self.objects = self.objects_all[1:cap + 1]
        self.header = self.fresh_header()
        nb = C.c_int64()
        N.call("dxrl_pg_val_levels_partial_doubles", L, G, K, C.byref(nb))
        self.partial_all = torch.full((nb.value + 2,), float("nan"), dtype=torch.float64, device=dev)
        self.partial = self.partial_all[1:nb.value + 1]
        o = params_offset  # 1: 4-byte aligned only (the scalar copy); 4: 16-byte aligned (float4 and a tail)
        self.params = torch.zeros(NP + o, device=dev)[o:]
        self.best_all = torch.full((NP + o + 8,), GUARD_P, device=dev)
        self.best = self.best_all[o:o + NP]

    def fresh_header(self):
        h = torch.zeros(64, dtype=torch.uint8, device=self.dev)
        h[8:24].view(torch.int64).fill_(-1)
        h[32:40].view(torch.float64).fill_(-math.inf)
        return h

    def set_records(self, **kw):
        for k, v in kw.items():
            if k == "status":
                self.status.fill_(int(v))
            else:
                self.t[k][:len(v)].copy_(torch.from_numpy(np.asarray(v)).to(self.dev))

    def args(self, row, iteration=3, env_steps=1234567, train_row=2, score_table=0, score_col=-1, min_delta=0.0,
             patience=0, solve_threshold=1.0, with_params=True, with_objects=True):
        N, d, p = self.N, self.data, self.N.ptr
        a = N.PgValLevelsArgs()
        a.num_levels, a.num_objects, a.episodes_per_object, a.row, a.cap = d["L"], d["G"], d["K"], row, self.cap
        a.iteration, a.env_steps, a.train_row = iteration, env_steps, train_row
        a.partial_doubles, a.score_table, a.score_col, a.patience = self.partial.numel(), score_table, score_col, patience
        a.min_delta, a.solve_threshold = min_delta, solve_threshold
        for k in ("ep_return", "ep_length", "ep_success", "ep_contacts"):
            setattr(a, k, p(self.t[k]))
        a.status, a.partial, a.val, a.header = p(self.status), p(self.partial), p(self.table), p(self.header)
        a.levels, a.robust, a.level_noise = p(self.levels), p(self.robust), p(self.noise)
        if with_objects:
            a.object_successes = p(self.objects)
        if with_params:
            a.num_params, a.params, a.best_params = NP, p(self.params), p(self.best)
        return a

    def call(self, row, **kw):
        a = self.args(row, **kw)
        self.N.call("dxrl_pg_val_levels_row", 0, C.byref(a), self.N.stream_of(self.dev))
        torch.cuda.synchronize()
        return self.table.cpu().numpy(), self.levels.cpu().numpy(), self.robust.cpu().numpy()

    def slice_row(self, l, score_col=-1, solve_threshold=1.0):
        """dxrl_pg_val_row with its record pointers offset by l G K: (row, object counts, header bytes)."""
        N, d, p, dev = self.N, self.data, self.N.ptr, self.dev
        G, K = d["G"], d["K"]
        a = N.PgValArgs()
        a.num_objects, a.episodes_per_object, a.row, a.cap = G, K, 0, 1
        a.iteration, a.env_steps, a.train_row = 3, 1234567, 2
        nb = C.c_int64()
        N.call("dxrl_pg_val_partial_doubles", G, K, C.byref(nb))
        partial = torch.zeros(nb.value, dtype=torch.float64, device=dev)
        table = torch.zeros(1, V.COLS, dtype=torch.float64, device=dev)
        objects = torch.zeros(1, G, dtype=torch.int32, device=dev)
        header = self.fresh_header()
        a.partial_doubles, a.score_col, a.solve_threshold = nb.value, score_col, solve_threshold
        for k in ("ep_return", "ep_length", "ep_success", "ep_contacts"):
            setattr(a, k, p(self.t[k][l * G * K:]))
        a.status, a.partial, a.val, a.header, a.object_successes = p(self.status), p(partial), p(table), p(header), \
            p(objects)
        N.call("dxrl_pg_val_row", 0, C.byref(a), N.stream_of(dev))
        torch.cuda.synchronize()
        return table.cpu().numpy()[0], objects.cpu().numpy()[0], header.cpu().numpy().tobytes()

    def head(self):
        from dexterous_rl_manipulation_amd.training_run import val_header_dict
        return val_header_dict(self.header.cpu().numpy())

    def assert_guards(self, rows_written, object_rows=None):
        """Nothing outside the written rows, the scratch and best_params' own elements changed."""
        keep = [r for r in range(self.cap + 2) if r - 1 not in rows_written]
        for t in (self.table_all, self.levels_all, self.robust_all):
            assert np.all(t.cpu().numpy()[keep] == FILL)
        keep = [r for r in range(self.cap + 2) if r - 1 not in (rows_written if object_rows is None else object_rows)]
        assert np.all(self.objects_all.cpu().numpy()[keep] == GUARD_I)
        b = self.best_all.cpu().numpy()
        off = self.best.storage_offset()
        assert np.all(b[:off] == GUARD_P) and np.all(b[off + NP:] == GUARD_P)
        p = self.partial_all.cpu().numpy()
        assert np.isnan(p[0]) and np.isnan(p[-1])

    def state_bytes(self):
        return tuple(x.cpu().numpy().tobytes() for x in (self.table, self.levels, self.robust, self.objects,
                                                         self.header))


LEVEL_EXACT = ("obs_noise_std", "dyn_noise_std", "episodes", "successes", "success_rate", "mean_length", "mean_contacts",
               "min_object_success_rate")
ROBUST_EXACT = ("levels", "worst_level", "worst_success_rate", "mean_success_rate", "mean_noisy_success_rate",
                "max_degradation", "max_degradation_percentage")
MAIN_STATS = ("episodes", "successes", "success_rate", "mean_return", "return_std", "mean_length", "mean_contacts",
              "min_object_success_rate")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,G,K", SHAPES)
def test_rows_against_the_restatement_and_the_single_set_kernel(N, L, G, K, kind):
    d = level_records(L, G, K, kind, seed=L + G + K)
    h = Harness(N, d)
    h.params.copy_(torch.arange(NP, device=h.dev, dtype=torch.float32) + 0.5)
    score_col = V.IDX["success_rate"]
    table, levels, robust = h.call(2, score_col=score_col)
    main, rows, rob = R.levels_row(d["noise"], G, K, 3, 1234567, 2, d["ep_return"], d["ep_length"], d["ep_success"],
                                   d["ep_contacts"], d["status"], 1.0)
    GK = G * K
    # the main row: level 0 against the restatement, by test_gpu_pg_val.py's check
    d0 = dict(G=G, K=K, ep_return=d["ep_return"][:GK])
    got_main = T.check_row(table[2], d0, main)
    # every level: exact columns, the two bounded ones, and the bytes of dxrl_pg_val_row on its slice
    counts = h.objects.cpu().numpy()[2]
    for l in range(L):
        got = {name: levels[2, l, k] for k, name in enumerate(R.LEVEL_COLUMNS)}
        ref = rows[l]
        for name in LEVEL_EXACT:
            assert got[name] == ref[name], (l, name)
        ret = d["ep_return"][l * GK:(l + 1) * GK]
        bound = T.sum_bound(ret) / GK
        print("level", l, "mean_return", got["mean_return"], ref["mean_return"], bound, "return_std", got["return_std"],
              ref["return_std"])
        assert abs(got["mean_return"] - ref["mean_return"]) <= bound
        if ref["return_std"] == 0.0:
            assert got["return_std"] == 0.0
        else:
            assert abs(got["return_std"] - ref["return_std"]) <= 1e-9 * ref["return_std"]
        assert counts[l].tolist() == V.object_successes(G, K, d["ep_success"][l * GK:(l + 1) * GK]).tolist()
        srow, scounts, sheader = h.slice_row(l, score_col=score_col)
        want = np.array([srow[V.IDX[name]] for name in MAIN_STATS])
        have = np.array([got[name] for name in MAIN_STATS])
        assert have.tobytes() == want.tobytes(), l
        assert counts[l].tobytes() == scounts.tobytes(), l
        if l == 0:  # the main row and, with score_table 0, the header: that call's bytes
            assert table[2].tobytes()[:V.IS_BEST * 8] == srow.tobytes()[:V.IS_BEST * 8]
            assert table[2, V.IS_BEST] == srow[V.IS_BEST] and table[2, V.SINCE_BEST] == srow[V.SINCE_BEST]
            hb = h.header.cpu().numpy().copy()
            sb = np.frombuffer(sheader, dtype=np.uint8).copy()
            # rows_written and best_row name the row: 3 / 2 here, 1 / 0 there
            assert hb[16:].tobytes() == sb[16:].tobytes()
    # degradation and robust columns from the device's own rates and returns: the restatement, ==
    dev_rows = R.add_degradation([{name: levels[2, l, k] for k, name in enumerate(R.LEVEL_COLUMNS)} for l in range(L)])
    assert R.nan_equal(levels[2], R.level_array(dev_rows))
    assert R.nan_equal(robust[2], R.robust_array(R.robust_values(dev_rows)))
    # and from the restatement's rates (exact), apart from worst_mean_return, which is bounded above
    for name in ROBUST_EXACT:
        assert R.nan_equal(robust[2, R.RIDX[name]], rob[name]), name
    assert R.nan_equal(levels[2][:, R.LIDX["degradation"]], [r["degradation"] for r in rows])
    assert R.nan_equal(levels[2][:, R.LIDX["degradation_percentage"]], [r["degradation_percentage"] for r in rows])
    assert levels[2, 0, R.LIDX["degradation"]] == 0.0 and levels[2, 0, R.LIDX["degradation_percentage"]] == 0.0
    if L == 1:
        assert math.isnan(robust[2, R.RIDX["mean_noisy_success_rate"]])
    if kind == "baseline_all_fail":
        assert np.all(levels[2][:, R.LIDX["degradation_percentage"]] == 0.0)
        assert robust[2, R.RIDX["max_degradation"]] == 0.0
    if kind == "one_level_all_fail" and L > 1:
        assert robust[2, R.RIDX["worst_success_rate"]] == 0.0
        assert levels[2, L - 1, R.LIDX["degradation"]] == levels[2, 0, R.LIDX["success_rate"]]
        if levels[2, 0, R.LIDX["success_rate"]] > 0:
            assert levels[2, L - 1, R.LIDX["degradation_percentage"]] == 100.0
    head = h.head()
    if kind == "bad_status":
        assert got_main["eval_status"] == 1.0 and got_main["is_best"] == 0.0 and head["best_row"] == -1
        assert torch.all(h.best == GUARD_P)
    else:
        assert got_main["is_best"] == 1.0 and head["best_row"] == 2 and head["best_score"] == main["success_rate"]
        assert torch.equal(h.best, h.params)
    assert head["rows_written"] == 3 and head["stopped_row"] == -1
    h.assert_guards({2})


@pytest.mark.parametrize("L,G,K", [(2, 3, 5), (3, 37, 33), (2, 67, 1001)])
def test_repeat_calls_and_base_offsets_give_the_same_bytes(N, L, G, K):
    d = level_records(L, G, K, "random", seed=5)
    out = []
    for offset in (0, 0, 1, 3):
        h = Harness(N, d, offset=offset)
        h.call(1, score_table=1, score_col=R.RIDX["mean_success_rate"], solve_threshold=0.5)
        out.append(h.state_bytes())
        h.assert_guards({1})
    assert out[0] == out[1] == out[2] == out[3]


def test_optional_outputs_and_no_score(N):
    d = level_records(3, 7, 7, "random", seed=1)
    h = Harness(N, d)
    table, levels, robust = h.call(0, with_params=False, with_objects=False)
    assert table[0, V.IS_BEST] == 0.0 and table[0, V.SINCE_BEST] == 1.0
    assert torch.all(h.best == GUARD_P)
    h.assert_guards({0}, object_rows=set())
    h2 = Harness(N, d)
    h2.call(0)  # params given, no score column: no copy
    assert torch.all(h2.best == GUARD_P) and h2.head()["best_row"] == -1
    assert h2.levels.cpu().numpy()[0].tobytes() == levels[0].tobytes()


def test_robust_columns_select_the_score(N):
    """Each robust column as the score: best_score is that column of the robust row."""
    d = level_records(5, 7, 7, "random", seed=2)
    for name in R.ROBUST_SCORES:
        h = Harness(N, d)
        _, _, robust = h.call(0, score_table=1, score_col=R.RIDX[name])
        assert h.head()["best_score"] == robust[0, R.RIDX[name]] and h.head()["best_row"] == 0
    h = Harness(N, level_records(1, 3, 5, "random", seed=2))
    table, _, robust = h.call(0, score_table=1, score_col=R.RIDX["mean_noisy_success_rate"])
    assert math.isnan(robust[0, R.RIDX["mean_noisy_success_rate"]])  # L = 1: a NaN score is never best
    assert table[0, V.IS_BEST] == 0.0 and h.head()["best_row"] == -1 and torch.all(h.best == GUARD_P)


def run_series(N, scores, statuses=None, min_delta=0.0, patience=0, score_col=WORST_RETURN):
    """Rows of 2 levels x 2 x 2 records: level 0's returns all scores[r] + 1, level 1's all
    scores[r], so worst_mean_return is exactly scores[r] and the main row's mean_return is not;
    params of row r = r + 1."""
    L, G, K = 2, 2, 2
    d = level_records(L, G, K, "random", seed=3)
    h = Harness(N, d, cap=len(scores), params_offset=4)
    want_best, want_header, want_flags = R.robust_series(scores, min_delta, patience if score_col >= 0 else 0, statuses)
    best_so_far = None
    for r, s in enumerate(scores):
        h.set_records(ep_return=np.concatenate([np.full(G * K, s + 1.0), np.full(G * K, s)]),
                      status=0 if statuses is None else statuses[r])
        h.params.fill_(float(r + 1))
        table, levels, robust = h.call(r, iteration=10 + r, score_table=1, score_col=score_col, min_delta=min_delta,
                                       patience=patience)
        assert R.nan_equal(robust[r, WORST_RETURN], s)
        if not math.isnan(s):
            assert table[r, V.IDX["mean_return"]] == s + 1.0
        if score_col >= 0:
            assert table[r, V.IS_BEST] == want_flags[r, 0] and table[r, V.SINCE_BEST] == want_flags[r, 1], r
            if r in want_best:
                best_so_far = r
        want = GUARD_P if best_so_far is None else float(best_so_far + 1)
        assert torch.all(h.best == want), r
        h.assert_guards(set(range(r + 1)))
    return h.head(), want_header, h.table.cpu().numpy()


def test_keep_best_on_a_robust_score_is_strict_and_the_first_maximum_wins(N):
    head, want, table = run_series(N, [1.0, 3.0, 3.0, 2.0, 9.0, 4.0])
    assert head == want and head["best_row"] == 4 and head["best_score"] == 9.0
    assert table[:, V.IS_BEST].tolist() == [1, 1, 0, 0, 1, 0]
    head, want, _ = run_series(N, [5.0, 5.0, 5.0])
    assert head == want and head["best_row"] == 0


def test_nan_score_and_bad_status_are_never_best(N):
    nan = float("nan")
    head, want, table = run_series(N, [1.0, nan, 2.0, nan])
    assert head == want and head["best_row"] == 2 and table[:, V.IS_BEST].tolist() == [1, 0, 1, 0]
    head, want, table = run_series(N, [nan, nan])
    assert head == want and head["best_row"] == -1 and head["best_score"] == -math.inf
    head, want, table = run_series(N, [1.0, 9.0, 2.0], statuses=[0, 1, 0])
    assert head == want and head["best_row"] == 2 and table[:, V.IDX["eval_status"]].tolist() == [0, 1, 0]


@pytest.mark.parametrize("min_delta,best", [(0.5 - 1e-12, [1, 1, 1, 1]), (0.5 + 1e-12, [1, 0, 1, 0]), (0.0, [1, 1, 1, 1])])
def test_min_delta_just_below_and_just_above_the_step(N, min_delta, best):
    head, want, table = run_series(N, [1.0, 1.5, 2.0, 2.5], min_delta=min_delta)
    assert head == want and table[:, V.IS_BEST].tolist() == best


def test_patience_is_reached_exactly_and_stopped_row_sticks(N):
    head, want, table = run_series(N, [1.0, 2.0, 2.0, 1.0, 5.0, 0.0, 0.0, 0.0], patience=2)
    assert head == want and head["stopped_row"] == 3 and head["best_row"] == 4 and head["rows_written"] == 8
    assert table[:, V.SINCE_BEST].tolist() == [0, 0, 1, 2, 0, 1, 2, 3]
    head, want, _ = run_series(N, [1.0, 2.0, 2.0, 3.0], patience=2)  # one short of the patience
    assert head == want and head["stopped_row"] == -1
    head, want, _ = run_series(N, [1.0, 0.0, 0.0], patience=1)
    assert head == want and head["stopped_row"] == 1


def test_without_a_score_column_nothing_is_best_and_nothing_is_copied(N):
    head, want, table = run_series(N, [1.0, 2.0, 3.0], score_col=-1)
    assert head["best_row"] == -1 and head["best_score"] == -math.inf and head["rows_written"] == 3
    assert table[:, V.IS_BEST].tolist() == [0, 0, 0] and table[:, V.SINCE_BEST].tolist() == [1, 2, 3]


BAD = [
    ("num_levels", dict(num_levels=0)), ("num_levels", dict(num_levels=17)), ("num_levels", dict(num_levels=-1)),
    ("num_objects", dict(num_objects=0)), ("num_objects", dict(episodes_per_object=0)),
    ("INT32_MAX", dict(num_objects=1 << 16, episodes_per_object=1 << 15)),
    ("INT32_MAX", dict(num_levels=16, num_objects=1 << 14, episodes_per_object=1 << 14)),
    ("outside the table", dict(row=-1)), ("outside the table", dict(row=4)), ("outside the table", dict(cap=0)),
    ("score_table", dict(score_table=2)), ("score_table", dict(score_table=-1)),
    ("score_col", dict(score_table=0, score_col=V.IS_BEST)), ("score_col", dict(score_table=0, score_col=V.COLS + 5)),
    ("score_col", dict(score_table=1, score_col=R.ROBUST_COLS)),
    ("score_col", dict(score_table=1, score_col=V.IDX["mean_contacts"])),
    ("patience", dict(patience=-1)),
    ("null episode records", dict(ep_return=None)), ("null episode records", dict(ep_length=None)),
    ("null episode records", dict(ep_success=None)), ("null episode records", dict(ep_contacts=None)),
    ("null episode records", dict(status=None)),
    ("null partial", dict(partial=None)), ("null partial", dict(val=None)), ("null partial", dict(header=None)),
    ("null levels", dict(levels=None)), ("null levels", dict(robust=None)), ("null levels", dict(level_noise=None)),
    ("go together", dict(params=None)), ("go together", dict(best_params=None)),
    ("num_params", dict(num_params=0)),
    ("partial holds", dict(partial_doubles=8)),
]


def test_invalid_arguments_return_before_any_launch_with_outputs_untouched(N):
    d = level_records(2, 3, 5, "random", seed=4)
    h = Harness(N, d)
    before = h.header.cpu().numpy().tobytes()
    for match, change in BAD:
        a = h.args(0, score_col=V.IDX["success_rate"])
        for k, v in change.items():
            setattr(a, k, v)
        with pytest.raises(ValueError, match=match):
            N.call("dxrl_pg_val_levels_row", 0, C.byref(a), N.stream_of(h.dev))
    torch.cuda.synchronize()
    h.assert_guards(set())
    assert h.header.cpu().numpy().tobytes() == before
    assert np.isnan(h.partial_all.cpu().numpy()).all()  # not even the scratch was written
