"""GPU: dxrl_pg_runs_summarize on crafted slabs (tests/pg_runs_cases.py: R = 6 runs, cap = 130 rows,
24 and 16 columns, run_rows in {0, 1, W - 1, W, 70, 130}) against the NumPy restatement
(tests/pg_runs_reference.py).

Tolerances, from this project's validation tests: every integer-valued column and every selected
value (final_window_mean's inputs are summed left to right on both sides; best, convergence_row,
x_at_convergence, min, max) is exact; means are within n 2^-52 sum|x| / n; standard deviations and
standard errors within 1e-9 relative; mean / standard error is the f64 quotient of the two written
columns.  A second call gives identical bytes; the canaries around every output buffer stay."""
import ctypes as C

import numpy as np
import pytest
import torch

import pg_runs_cases as K
import pg_runs_reference as P

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GUARD, CANARY = 16, -7.25e77


@pytest.fixture(scope="module")
def native():
    from dexterous_rl_manipulation_amd import _native
    _native.lib()
    return _native


def guarded(n, dev):
    t = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float64, device=dev)
    return t, t[GUARD:GUARD + n]


def summarize(native, tables, run_rows, specs, off, flat, weights, num_members=None):
    """One call on device copies of the inputs, outputs between canaries: the three tables, the
    status and the raw bytes of everything written."""
    dev = torch.device("cuda", torch.cuda.current_device())
    R, cap, cols = tables.shape
    S, G, Q = len(specs), len(off) - 1, len(weights)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    t_d, rows_d, off_d = up(tables, np.float64), up(run_rows, np.int32), up(off, np.int32)
    flat_d = up(np.concatenate([flat, [0]]), np.int32)  # never empty
    w_d = up(np.asarray(weights, dtype=np.float64).reshape(Q, G) if Q else np.zeros(1), np.float64)
    sizes = (R * S * P.RUN_COLS, G * S * P.METRICS * P.GROUP_COLS, Q * S * P.METRICS * P.CONTRAST_COLS)
    bufs = [guarded(n, dev) for n in sizes]
    status = torch.full((3,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    nat = (native.PgRunsSpec * S)()
    for k, (col, x_col, w, thr, fw) in enumerate(specs):
        nat[k].col, nat[k].x_col, nat[k].window, nat[k].threshold, nat[k].final_window = col, x_col, w, thr, fw
    a = native.PgRunsArgs()
    a.num_runs, a.cap, a.cols, a.num_specs, a.num_groups, a.num_contrasts = R, cap, cols, S, G, Q
    a.num_members = len(flat) if num_members is None else num_members
    a.specs = nat
    a.tables, a.run_rows, a.group_offsets, a.group_runs = t_d.data_ptr(), rows_d.data_ptr(), off_d.data_ptr(), \
        flat_d.data_ptr()
    a.contrast_weights = w_d.data_ptr()
    a.run_table, a.group_table, a.contrast_table = (b[1].data_ptr() for b in bufs)
    a.status = status[1:].data_ptr()
    native.call("dxrl_pg_runs_summarize", dev.index, C.byref(a), native.stream_of(dev))
    torch.cuda.synchronize()
    for whole, _ in bufs:
        w = whole.cpu().numpy()
        assert (w[:GUARD] == CANARY).all() and (w[-GUARD:] == CANARY).all()
    st = status.cpu().numpy()
    assert st[0] == st[2] == 0x5a5a5a5a
    shapes = ((R, S, P.RUN_COLS), (G, S, P.METRICS, P.GROUP_COLS), (Q, S, P.METRICS, P.CONTRAST_COLS))
    out = [b[1].cpu().numpy().reshape(shape) for b, shape in zip(bufs, shapes)]
    return out[0], out[1], out[2], int(st[1])


@pytest.mark.parametrize("cols", [24, 16], ids=["log_cols", "val_cols"])
def test_crafted_slab_equals_the_restatement_and_repeats_bit_for_bit(native, cols):
    tables = K.slab(cols)
    off, flat = K.csr()
    want = P.summarize(tables, K.RUN_ROWS, K.SPECS, off, flat, K.CONTRASTS)
    got = summarize(native, tables, K.RUN_ROWS, K.SPECS, off, flat, K.CONTRASTS)
    P.check_tables(got, want, tables, K.RUN_ROWS, K.SPECS, off, flat, K.CONTRASTS)
    run, grp, con, status = got
    assert status == P.ST_CONTRAST and np.isnan(con[K.Q_UNEQUAL]).all()
    assert not np.isin(K.SENTINEL, run)  # nothing past run_rows[r] was read into a statistic
    # the crafted values themselves
    c = run[K.CRAFTED, 0]
    assert c[P.CONV] == 43 and c[P.X_AT_CONV] == 44000.0  # rows 20 .. 23 sit exactly on the threshold
    assert c[P.BEST] == 0.625 and c[P.BEST_ROW] == 43     # row 60 holds the same maximum
    assert c[P.NAN_ROWS] == 1 and np.isnan(run[K.CRAFTED, 1, P.FINAL])
    assert run[K.NEVER, 0, P.CONV] == -1 and run[K.SHORT, 0, P.CONV] == -1 and run[K.EXACT_W, 0, P.CONV] == K.W - 1
    assert run[K.EMPTY, 0].tolist()[3:5] == [-1.0, -1.0] and np.isnan(run[K.EMPTY, 0, [1, 2, 5, 6]]).all()
    g = K.NAMES.index("none_converged")
    assert grp[g, 0, P.M_CONV, 0] == 0 and grp[g, 0, P.M_FINAL, 5] == 0 and grp[g, 0, P.M_FINAL, 0] == 2
    assert (grp[K.NAMES.index("empty"), :, :, 0] == 0).all()
    assert con[K.Q_NAN_MEMBER, 0, P.M_FINAL, 0] == 1      # the empty run's pair is left out
    # determinism: the same inputs, the same bytes
    again = summarize(native, tables, K.RUN_ROWS, K.SPECS, off, flat, K.CONTRASTS)
    for a, b in zip(got[:3], again[:3]):
        assert a.tobytes() == b.tobytes()
    assert again[3] == status


def test_out_of_range_members_offsets_and_rows_are_skipped_and_reported(native):
    tables = K.slab(16)
    rows = K.RUN_ROWS.copy()
    rows[K.ONE], rows[K.SHORT] = -1, K.CAP + 1
    groups = {"bad": [K.CRAFTED, K.R, -1, K.NEVER], "good": [K.CRAFTED, K.NEVER], "far": [2 ** 31 - 1, K.EXACT_W],
              "short": [K.ONE, K.SHORT]}
    off, flat = K.csr(groups)
    weights = np.array([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, -1.0]])
    # bad against far: 4 members against 2 (bit 2); good against short: two pairs of which none is finite
    want = P.summarize(tables, rows, K.SPECS, off, flat, weights)
    got = summarize(native, tables, rows, K.SPECS, off, flat, weights)
    assert got[3] == want[3] == P.ST_RANGE | P.ST_ROWS | P.ST_CONTRAST
    P.check_tables(got, want, tables, rows, K.SPECS, off, flat, weights)
    run, grp, con, _ = got
    assert (run[[K.ONE, K.SHORT], :, P.ROWS] == 0).all()
    assert P.same(grp[0], grp[1])  # the members in range, at their places: the same statistics
    assert (con[1, :, P.M_FINAL, 0] == 0).all()
    # offsets past the member list (num_members says where it ends) and offsets that decrease
    for bad_off, members in ((np.array([0, 2, 9], dtype=np.int32), 4), (np.array([2, 1, 3], dtype=np.int32), 4)):
        flat4 = np.array([K.CRAFTED, K.NEVER, K.EXACT_W, K.ONE], dtype=np.int32)
        w = np.array([[1.0, -1.0]])
        got = summarize(native, tables, K.RUN_ROWS, K.SPECS, bad_off, flat4, w, num_members=members)
        want = P.summarize(tables, K.RUN_ROWS, K.SPECS, bad_off, flat4, w)
        assert got[3] == want[3] == P.ST_RANGE | P.ST_CONTRAST
        P.check_tables(got, want, tables, K.RUN_ROWS, K.SPECS, bad_off, flat4, w)
        assert np.isnan(got[2]).all()


def test_run_pass_alone_and_many_members(native):
    """G = Q = 0 launches the run pass only; a group of 150 members wraps the wave loop of the
    group and contrast passes."""
    tables = K.slab(24, seed=3)
    got = summarize(native, tables, K.RUN_ROWS, K.SPECS[:1], np.zeros(1, dtype=np.int32), np.zeros(0, np.int32), [])
    want = P.summarize(tables, K.RUN_ROWS, K.SPECS[:1])
    assert got[3] == want[3] == 0 and got[1].size == 0 and got[2].size == 0
    P.check_tables(got, want, tables, K.RUN_ROWS, K.SPECS[:1], [0], [], [])
    rng = np.random.default_rng(5)
    groups = {"x": rng.integers(1, K.R, 150).tolist(), "y": rng.integers(1, K.R, 150).tolist()}
    off, flat = K.csr(groups)
    w = np.array([[1.0, -1.0], [0.5, 0.5]])
    got = summarize(native, tables, K.RUN_ROWS, K.SPECS, off, flat, w)
    want = P.summarize(tables, K.RUN_ROWS, K.SPECS, off, flat, w)
    assert got[3] == want[3] == 0 and got[1][0, 0, P.M_FINAL, 0] == 150
    P.check_tables(got, want, tables, K.RUN_ROWS, K.SPECS, off, flat, w)
