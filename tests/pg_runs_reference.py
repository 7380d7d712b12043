"""NumPy restatement of dxrl_pg_runs_summarize (include/dxrl.h), pass by pass, in the orders the
header states: left-to-right window sums, the lane-strided curve sum with its 32, 16, .., 1 tree,
Welford steps per wave lane and Chan et al.'s merge in the same tree.  A spec is the tuple
(col, x_col, window, threshold, final_window)."""
import math

import numpy as np

WAVE = 64
RUN_COLS, METRICS, GROUP_COLS, CONTRAST_COLS = 8, 5, 6, 5
ROWS, FINAL, BEST, BEST_ROW, CONV, X_AT_CONV, CURVE_MEAN, NAN_ROWS = range(8)
METRIC_RUN_COL = (FINAL, BEST, CONV, X_AT_CONV, CURVE_MEAN)  # enum dxrl_pg_runs_metric
M_FINAL, M_BEST, M_CONV, M_X, M_CURVE = range(5)
ST_RANGE, ST_ROWS, ST_CONTRAST = 1, 2, 4
NAN = float("nan")


def left_to_right(values):
    s = 0.0
    for x in values:
        s = s + float(x)
    return s


def tree(lanes, combine):
    lanes = list(lanes)
    o = WAVE // 2
    while o >= 1:
        for t in range(o):
            lanes[t] = combine(lanes[t], lanes[t + o])
        o //= 2
    return lanes[0]


def welford(m, x):
    n, mean, m2 = m
    n1 = n + 1.0
    d = x - mean
    mean = mean + d / n1
    return (n1, mean, m2 + d * (x - mean))


def chan(a, b):
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n = a[0] + b[0]
    d = b[1] - a[1]
    return (n, a[1] + d * (b[0] / n), a[2] + b[2] + d * d * (a[0] * b[0] / n))


def lane_moments(values):
    """(count, mean, M2) of the finite entries of `values` (None = no value at that position):
    position j is a Welford step of lane j % 64."""
    lanes = [(0.0, 0.0, 0.0)] * WAVE
    for j, x in enumerate(values):
        if x is not None and math.isfinite(x):
            lanes[j % WAVE] = welford(lanes[j % WAVE], float(x))
    return tree(lanes, chan)


def run_row(v, x, spec):
    _, _, W, thr, FW = spec
    n = len(v)
    out = [float(n), NAN, NAN, -1.0, -1.0, NAN, NAN, 0.0]
    k = min(FW, n)
    if k > 0:
        out[FINAL] = left_to_right(v[n - k:]) / k
    lanes = [0.0] * WAVE
    count = 0
    for i in range(n):
        if math.isnan(v[i]):
            out[NAN_ROWS] += 1.0
            continue
        if out[BEST_ROW] < 0 or v[i] > out[BEST]:
            out[BEST], out[BEST_ROW] = float(v[i]), float(i)
        lanes[i % WAVE] = lanes[i % WAVE] + float(v[i])
        count += 1
    if count:
        out[CURVE_MEAN] = tree(lanes, lambda a, b: a + b) / count
    for i in range(W - 1, n):
        if left_to_right(v[i - W + 1:i + 1]) / W > thr:
            out[CONV], out[X_AT_CONV] = float(i), float(x[i])
            break
    return out


def run_pass(tables, run_rows, specs):
    tables = np.asarray(tables, dtype=np.float64)
    R, cap, _ = tables.shape
    out = np.zeros((R, len(specs), RUN_COLS))
    status = 0
    for r in range(R):
        n = int(run_rows[r])
        if n < 0 or n > cap:
            status |= ST_ROWS
            n = 0
        for s, spec in enumerate(specs):
            out[r, s] = run_row(tables[r, :n, spec[0]], tables[r, :n, spec[1]], spec)
    return out, status


def metrics_of(row):
    x = [float(row[c]) for c in METRIC_RUN_COL]
    if row[CONV] < 0:
        x[M_CONV] = NAN
    return x


def group_members(offsets, members, g):
    lo, hi = int(offsets[g]), int(offsets[g + 1])
    if lo < 0 or hi < lo or hi > len(members):
        return None
    return [int(r) for r in members[lo:hi]]


def group_pass(run_table, offsets, members):
    R, S, _ = run_table.shape
    G = len(offsets) - 1
    out = np.full((G, S, METRICS, GROUP_COLS), NAN)
    status = 0
    for g in range(G):
        mem = group_members(offsets, members, g)
        if mem is None:
            status |= ST_RANGE
            mem = []
        if any(not 0 <= r < R for r in mem):
            status |= ST_RANGE
        for s in range(S):
            rows = [metrics_of(run_table[r, s]) if 0 <= r < R else None for r in mem]
            converged = sum(1 for r in mem if 0 <= r < R and run_table[r, s, CONV] >= 0)
            for k in range(METRICS):
                vals = [None if m is None else m[k] for m in rows]
                n, mean, m2 = lane_moments(vals)
                out[g, s, k, 0], out[g, s, k, 5] = n, converged
                if n:
                    fin = [v for v in vals if v is not None and math.isfinite(v)]
                    out[g, s, k, 1:5] = mean, math.sqrt(m2 / n), min(fin), max(fin)
    return out, status


def contrast_pass(run_table, offsets, members, weights):
    R, S, _ = run_table.shape
    G = len(offsets) - 1
    weights = np.asarray(weights, dtype=np.float64)
    weights = weights.reshape(-1, G) if G else np.zeros((0, 0))
    out = np.full((len(weights), S, METRICS, CONTRAST_COLS), NAN)
    status = 0
    for q, w in enumerate(weights):
        used = [g for g in range(G) if w[g] != 0.0]
        mems = [group_members(offsets, members, g) for g in used]
        if any(m is None for m in mems) or len({len(m) for m in mems}) > 1:
            status |= ST_CONTRAST
            continue
        m = len(mems[0]) if mems else 0
        for s in range(S):
            for k in range(METRICS):
                d = []
                for j in range(m):
                    terms = [w[g] * metrics_of(run_table[mem[j], s])[k] if 0 <= mem[j] < R else NAN
                             for g, mem in zip(used, mems)]
                    d.append(left_to_right(terms) if all(math.isfinite(t) for t in terms) else None)
                n, mean, m2 = lane_moments(d)
                out[q, s, k, 0] = n
                if n:
                    sd = math.sqrt(m2 / (n - 1.0)) if n >= 2 else NAN
                    se = sd / math.sqrt(n)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        out[q, s, k, 1:] = mean, sd, se, np.float64(mean) / np.float64(se)
    return out, status


EPS = 2.0 ** -52


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check_tables(got, want, tables, run_rows, specs, off, flat, weights):
    """(run_table, group_table, contrast_table, status) `got` against the restatement's `want`:
    the status, every integer-valued column and every selected value exact; means within
    n 2^-52 sum|x| / n of their inputs; standard deviations and standard errors within 1e-9
    relative; mean / standard error the f64 quotient of the two written columns.  Prints each
    bounded figure before it asserts."""
    run, grp, con, status = got
    ref_run, ref_grp, ref_con, ref_status = want
    assert status == ref_status
    exact = [ROWS, FINAL, BEST, BEST_ROW, CONV, X_AT_CONV, NAN_ROWS]  # everything but curve_mean
    assert same(run[:, :, exact], ref_run[:, :, exact])
    assert same(np.isnan(run), np.isnan(ref_run))
    R = len(run)
    for r in range(R):
        n = int(run_rows[r]) if 0 <= run_rows[r] <= tables.shape[1] else 0
        for s, spec in enumerate(specs):
            v = tables[r, :n, spec[0]]
            v = v[~np.isnan(v)]
            if v.size:
                bound = v.size * EPS * np.abs(v).sum() / v.size
                print("curve_mean", r, s, run[r, s, CURVE_MEAN], ref_run[r, s, CURVE_MEAN], bound)
                assert abs(run[r, s, CURVE_MEAN] - ref_run[r, s, CURVE_MEAN]) <= bound
    # group rows: count, min, max and converged runs exact; mean and std within their bounds
    assert same(np.isnan(grp), np.isnan(ref_grp))
    assert same(grp[..., [0, 3, 4, 5]], ref_grp[..., [0, 3, 4, 5]])
    G, S = grp.shape[0], run.shape[1]
    for g in range(G):
        mem = group_members(off, flat, g) or []
        for s in range(S):
            for k in range(METRICS):
                x = np.array([metrics_of(ref_run[r, s])[k] for r in mem if 0 <= r < R])
                x = x[np.isfinite(x)]
                if x.size:
                    print("group", g, s, k, grp[g, s, k, 1:3], ref_grp[g, s, k, 1:3])
                    assert abs(grp[g, s, k, 1] - ref_grp[g, s, k, 1]) <= x.size * EPS * np.abs(x).sum() / x.size
                    assert abs(grp[g, s, k, 2] - ref_grp[g, s, k, 2]) <= 1e-9 * ref_grp[g, s, k, 2]
    # contrast rows: pairs exact, mean / std / stderr within their bounds, t the quotient
    assert same(np.isnan(con), np.isnan(ref_con))
    assert same(con[..., 0], ref_con[..., 0])
    for q in range(len(con)):
        used = [g for g in range(G) if weights[q][g] != 0.0]
        for s in range(S):
            for k in range(METRICS):
                row, ref = con[q, s, k], ref_con[q, s, k]
                if not ref[0] > 0:
                    continue
                # sum|d| <= sum over the weighted groups of |w| |x|
                total = sum(abs(weights[q][g]) * abs(metrics_of(ref_run[r, s])[k])
                            for g in used for r in group_members(off, flat, g)
                            if 0 <= r < R and math.isfinite(metrics_of(ref_run[r, s])[k]))
                print("contrast", q, s, k, row, ref)
                assert abs(row[1] - ref[1]) <= ref[0] * EPS * total / ref[0]
                if ref[0] >= 2:
                    assert abs(row[2] - ref[2]) <= 1e-9 * ref[2] and abs(row[3] - ref[3]) <= 1e-9 * ref[3]
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = np.float64(row[1]) / np.float64(row[3])
                assert row[4] == t or (np.isnan(row[4]) and np.isnan(t))


def summarize(tables, run_rows, specs, offsets=(0,), members=(), weights=None):
    """All three passes: (run_table, group_table, contrast_table, status)."""
    run_table, st = run_pass(tables, run_rows, specs)
    group_table, st_g = group_pass(run_table, offsets, members)
    G = len(offsets) - 1
    weights = np.zeros((0, G)) if weights is None else weights
    contrast_table, st_c = contrast_pass(run_table, offsets, members, weights)
    return run_table, group_table, contrast_table, st | st_g | st_c
