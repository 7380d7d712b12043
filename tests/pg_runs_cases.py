"""Crafted slabs for dxrl_pg_runs_summarize, shared by the CPU and the GPU tests: R = 6 runs of up to
cap = 130 rows (the wave loop wraps twice and ends in a ragged tail), values that are multiples of
1 / 8 so that a window of W = 4 can sit exactly on the threshold, and rows past run_rows[r] filled
with a sentinel no statistic may contain."""
import numpy as np

R, CAP, W, THR = 6, 130, 4, 0.5
RUN_ROWS = np.array([0, 1, W - 1, W, 70, 130], dtype=np.int32)
SENTINEL = 1.0e300
EMPTY, ONE, SHORT, EXACT_W, CRAFTED, NEVER = range(R)  # the runs, by run_rows
# (col, x_col, window, threshold, final_window)
SPECS = ((5, 1, W, THR, 10),     # the crafted column
         (3, 0, W, THR, 3),      # a NaN inside the final window of run CRAFTED
         (4, 1, 1, 0.75, 200),   # W = 1; a final window longer than every run
         (2, 1, 64, 0.1, 64))    # a window as long as the wave


def slab(cols: int, seed: int = 0) -> np.ndarray:
    """f64 [R][CAP][cols]: column 0 the row index, column 1 'env steps', the others multiples of
    1 / 8 in [0, 1] with NaN rows sprinkled in; column 5 crafted (below)."""
    rng = np.random.default_rng(seed + cols)
    t = rng.integers(0, 9, size=(R, CAP, cols)).astype(np.float64) / 8.0
    t[rng.random((R, CAP, cols)) < 0.04] = np.nan
    t[:, 0] = np.nan_to_num(t[:, 0], nan=0.375)  # every run that has a row has a value in every column
    t[:, :, 0] = np.arange(CAP)
    t[:, :, 1] = 1000.0 * (np.arange(CAP) + 1)
    v = t[:, :, 5]
    v[ONE, 0] = 0.875
    v[SHORT, :3] = [1.0, 1.0, 1.0]          # W - 1 rows: no window, however good
    v[EXACT_W, :4] = [0.75, 0.75, 0.5, 0.25]  # mean 0.5625 > 0.5 at row W - 1, the only window
    c = v[CRAFTED]
    c[:70] = 0.25
    c[10] = np.nan                          # a NaN row outside the final window (rows 60 .. 69)
    c[20:24] = 0.5                          # a window mean exactly on the threshold: not converged
    c[40:44] = [0.5, 0.5, 0.5, 0.625]       # 0.53125: the first window above it ends at row 43
    c[60] = 0.625                           # the maximum again: the first one (row 43) wins
    t[CRAFTED, 68, 3] = np.nan              # spec 1: a NaN inside its final window (rows 67 .. 69)
    t[CRAFTED, 50, 3] = 0.5
    nv = rng.integers(0, 5, size=CAP).astype(np.float64) / 8.0  # <= 0.5: a mean never strictly above it
    nv[30:40] = 0.5
    nv[77] = np.nan
    v[NEVER] = nv
    for r in range(R):
        t[r, RUN_ROWS[r]:] = SENTINEL
    return t


# CSR groups over the runs: overlapping ones, an empty one, one whose runs all failed to converge
# on spec 0 (SHORT has no window, NEVER stays at or below the threshold), one with the empty run
# (its metrics are NaN) and one of another size
GROUPS = {"a": [EXACT_W, CRAFTED], "b": [CRAFTED, NEVER], "empty": [], "none_converged": [NEVER, SHORT],
          "with_empty_run": [EMPTY, ONE], "three": [EXACT_W, CRAFTED, NEVER], "d": [ONE, EXACT_W]}
NAMES = list(GROUPS)


def csr(groups=None):
    m = list((GROUPS if groups is None else groups).values())
    off = np.zeros(len(m) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in m])
    flat = np.array([r for x in m for r in x], dtype=np.int32)
    return off, flat


def weights(rows):
    w = np.zeros((len(rows), len(NAMES)))
    for q, row in enumerate(rows):
        for name, x in row.items():
            w[q, NAMES.index(name)] = x
    return w


# the three factorial rows over the 2 x 2 (a, b, none_converged, d), a contrast with a NaN member,
# one whose groups differ in size (status bit 2, NaN rows) and one that weighs nothing
CONTRASTS = weights([
    {"a": 0.5, "b": 0.5, "none_converged": -0.5, "d": -0.5},
    {"a": 0.5, "none_converged": 0.5, "b": -0.5, "d": -0.5},
    {"a": 1.0, "b": -1.0, "none_converged": -1.0, "d": 1.0},
    {"a": 1.0, "with_empty_run": -1.0},
    {"a": 1.0, "three": -1.0},
    {},
])
Q_NAN_MEMBER, Q_UNEQUAL, Q_NOTHING = 3, 4, 5
