"""Record sets for the dxrl_study_summarize tests (host and GPU): randomised runs and crafted
edge records, each a dict of [N][cap] buffers as dxrl_rollout_curriculum writes them.  The cells
past a lane's episode count hold sentinels (NaN returns, negative lengths, success 1) that a
correct reader never touches."""
import functools

import numpy as np

W, C_MIN, THR = 20, 10, 0.5
E_SIZES = [1, 12, 19, 20, 21, 64, 65, 70, 200]


def _buffers(rows, cap, levels=True):
    n = len(rows)
    ret = np.full((n, cap), np.nan)
    length = np.full((n, cap), -7, dtype=np.int32)
    success = np.ones((n, cap), dtype=np.uint8)
    level = np.full((n, cap), -3, dtype=np.int32)
    eps = np.zeros(n, dtype=np.int32)
    for l, (r, s, ok) in enumerate(rows):
        E = len(r)
        eps[l] = E
        ret[l, :E], length[l, :E], success[l, :E] = r, s, ok
        level[l, :E] = np.minimum(np.arange(E) // 9, 5)
    return {"ep_return": ret, "ep_length": length, "ep_success": success, "ep_level": level if levels else None,
            "episodes": eps, "cap": cap}


def _random_rows(seed, sizes, p):
    rng = np.random.default_rng(seed)
    rows = []
    for k, E in enumerate(sizes):
        # returns drift across the threshold in some lanes and stay on one side in others
        base = rng.uniform(-2.0, 2.0) + np.linspace(0.0, rng.uniform(-3.0, 3.0), E)
        rows.append((base + rng.normal(0.0, 0.7, E), rng.integers(1, 51, E), rng.random(E) < p[k % len(p)]))
    return rows


@functools.lru_cache(None)
def random_ragged():
    """16 lanes, every E at which the lane pass takes another path, record_cap > E."""
    sizes = E_SIZES + [200, 70, 65, 33, 128, 129, 5]
    return _buffers(_random_rows(7, sizes, (0.3, 0.55, 0.7)), 208)


@functools.lru_cache(None)
def random_uniform():
    """12 lanes of 70 episodes (three arms of four seeds): the group tables' integer form applies."""
    return _buffers(_random_rows(11, [70] * 12, (0.2, 0.5, 0.8)), 70, levels=False)


def _ok(E, idx):
    s = np.zeros(E, dtype=bool)
    s[list(idx)] = True
    return s


CRAFTED = ["conv_at_w", "conv_at_last", "nine_of_20", "ten_of_20", "straddle_64", "E_eq_w", "E_lt_w", "zero_mean",
           "all_thr", "cross_late"]


@functools.lru_cache(None)
def crafted():
    """One lane per edge (names in CRAFTED), window 20."""
    rng = np.random.default_rng(3)

    def ret(E):
        return rng.uniform(1.0, 2.0, E)  # moving averages far above the threshold: reward convergence at w - 1

    def steps(E):
        return rng.integers(1, 41, E)

    late = np.concatenate([np.full(30, -1.0), np.full(30, 2.5)])  # ma_18 = 0.4, ma_19 = 0.575: reported as 38
    rows = [
        (ret(40), steps(40), _ok(40, range(0, 20, 2))),      # 10 of the first 20: converged at i = w
        (ret(40), steps(40), _ok(40, range(29, 39))),        # window [19, 39) is the first with 10: i = E - 1
        (ret(40), steps(40), _ok(40, range(9))),             # 9 of 20 at most: never
        (ret(40), steps(40), _ok(40, range(10))),            # 10 of 20: at i = 20
        (ret(80), steps(80), _ok(80, range(55, 67))),        # the first window with 10 is [45, 65): straddles 64
        (ret(20), steps(20), _ok(20, range(20))),            # E == w: the loop is empty
        (ret(7), steps(7), _ok(7, (1, 2, 6))),               # E < w
        (np.zeros(40), steps(40), _ok(40, ())),              # mean reward exactly 0: CV infinite
        (np.full(40, THR), steps(40), _ok(40, range(5))),    # every moving average within rounding of thr
        (late, steps(60), _ok(60, range(40, 60))),
    ]
    return _buffers(rows, 80)


def lane_records(case, l):
    E = int(case["episodes"][l])
    return case["ep_return"][l, :E], case["ep_length"][l, :E], case["ep_success"][l, :E].astype(bool)
