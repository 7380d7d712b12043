"""NumPy / plain-Python restatement of ``dxrl_eval_summarize`` (csrc/dxrl_eval_summary.hip) and
the synthetic record sets its tests share.

``episode_pass`` is the per-episode launch written one episode at a time in Python integers
(independent of metrics.classify_columns, which tests compare it with); ``group_pass`` is the
per-group launch with a two-pass f64 mean / M2.  Tie rows -- integer variance exactly 2.0 at the
variance rule -- are classified as not unstable and flagged, as the kernel does; the host settles
them (evaluator.settle_ties).
"""
import numpy as np

SLIPPAGE, UNSTABLE, MISALIGNED, TIMEOUT, DROPPED, INSUFFICIENT = range(6)  # list(metrics.FailureType) order


def episode_pass(length, success, contacts, hist, max_steps, success_threshold=3):
    E = len(length)
    code = np.full(E, -1, np.int8)
    mom = np.zeros((E, 4), np.int32)
    tie = np.zeros(E, bool)
    for e in range(E):
        n = int(length[e])
        row = [int(c) for c in hist[e, :n]]
        s1, s2 = sum(row), sum(c * c for c in row)
        f5, l5 = sum(row[:5]), sum(row[-5:]) if n else 0
        mom[e] = s1, s2, f5, l5
        if success[e]:
            continue
        nc = int(contacts[e])
        if n >= max_steps:
            code[e] = TIMEOUT
        elif nc == 0:
            code[e] = DROPPED
        else:
            num, lim = n * s2 - s1 * s1, 2 * n * n
            tie[e] = n > 5 and num == lim
            if n > 5 and num > lim:
                code[e] = UNSTABLE
            elif n > 10 and (np.float64(l5) / 5.0) - (np.float64(f5) / 5.0) < -1.0:
                code[e] = SLIPPAGE
            elif 0 < nc < success_threshold:
                code[e] = MISALIGNED
            else:
                code[e] = INSUFFICIENT
    return code, mom, tie


def group_pass(code, tie, length, success, contacts, ret, groups):
    G = len(groups)
    stats = np.zeros((G, 16), np.int64)
    gret = np.zeros((G, 3))
    for g, idx in enumerate(groups):
        idx = np.asarray(idx, dtype=np.int64)
        if not len(idx):
            continue
        n = length[idx].astype(np.int64)
        ok = success[idx].astype(bool)
        c = contacts[idx].astype(np.int64)
        stats[g, :7] = len(idx), ok.sum(), n.sum(), (n * n).sum(), c.sum(), n[ok].sum(), c[ok].sum()
        stats[g, 7:13] = [(code[idx] == k).sum() for k in range(6)]
        stats[g, 13] = tie[idx].sum()
        r = ret[idx].astype(np.float64)
        gret[g] = len(idx), np.mean(r), np.sum((r - np.mean(r)) ** 2)
    return stats, gret


def _spread(total, parts=5):
    """`parts` counts in 0..5 summing to `total` (0..25), as even as possible."""
    base, rem = divmod(total, parts)
    return [base + 1] * rem + [base] * (parts - rem)


def var_tie_rows(want=3, seed=2024, max_n=30):
    """Count rows whose integer variance is exactly 2.0 with a non-integer mean (searched), at
    least one of which np.var rounds above 2.0: the rows the host fix-up has to move."""
    rng = np.random.default_rng(seed)
    ups, others = [], []
    for _ in range(200000):
        if ups and len(others) >= want - 1:
            break
        n = int(rng.integers(6, max_n))
        c = rng.integers(0, 6, n)
        if n * int((c * c).sum()) - int(c.sum()) ** 2 == 2 * n * n and int(c.sum()) % n:
            (ups if np.var(c.astype(np.int64)) > 2.0 else others).append(c.tolist())
    assert ups, "no tie row that np.var rounds above 2.0 was found"
    return others[:want - 1] + ups[:1]


def synthetic_rules(max_steps, n_pairs, seed=7):
    """Records that reach every rule and every edge of dxrl_eval_summarize's per-episode pass.
    Returns dict(length i32, success u8, contacts u8, ret f64, hist u8 [E][max_steps])."""
    rng = np.random.default_rng(seed + 1000 * max_steps + n_pairs)
    rows = []  # (history, success, contacts)

    def add(h, success=0, contacts=3):
        rows.append((list(h), success, contacts))

    # every (F, L) pair of first-five / last-five sums at history length n_pairs
    for F in range(26):
        for L in range(26):
            mid = [int(round((F + L) / 10.0))] * (n_pairs - 10)
            add(_spread(F) + mid + _spread(L)[::-1])
    # lengths around the rule thresholds, with every kind of closing rule
    for n in (1, 5, 6, 10, 11, max_steps):
        for _ in range(6):
            add(rng.integers(0, 6, n), success=int(rng.random() < 0.3), contacts=int(rng.integers(0, 6)))
        add([2] * n, contacts=3)                       # constant row: variance 0
        add([1] * n, success=1, contacts=4)            # success
        add([3] * n, contacts=0)                       # object dropped
        for nc in (1, 2, 3):
            add([nc] * n, contacts=nc)                 # misaligned (1, 2) / insufficient (3)
    # exact ties of the variance rule: open (contacts > 0), open with a misaligned provisional code,
    # and already closed by an earlier rule (success, dropped)
    ties = [[0, 0, 0, 0, 3, 3], [3, 3, 0, 0, 0, 0, 0, 0, 3]]
    add(ties[0], contacts=3)
    add(ties[1], contacts=1)
    for h in ties:
        add(h, success=1, contacts=3)
        add(h, contacts=0)
    for h in var_tie_rows(want=2):
        add(h, contacts=3)
    add([0, 0, 0, 0, 3, 4])                            # just above the tie
    add([0, 0, 0, 1, 3, 3])                            # just below
    add([0, 0, 0, 0, 0, 3, 3, 3, 3, 3, 3, 0])          # unstable before slippage can look
    for _ in range(40):                                # random histories of random lengths
        n = int(rng.integers(1, max_steps + 1))
        add(rng.integers(0, 6, n), success=int(rng.random() < 0.2), contacts=int(rng.integers(0, 6)))
    E = len(rows)
    hist = rng.integers(0, 256, (E, max_steps)).astype(np.uint8)  # garbage past each row's length
    length = np.zeros(E, np.int32)
    for e, (h, _, _) in enumerate(rows):
        length[e] = len(h)
        hist[e, :len(h)] = h
    return dict(length=length, success=np.array([r[1] for r in rows], np.uint8),
                contacts=np.array([r[2] for r in rows], np.uint8), ret=rng.normal(0.0, 10.0, E), hist=hist)


def random_records(E, max_steps, seed=5):
    rng = np.random.default_rng(seed)
    length = rng.integers(1, max_steps + 1, E).astype(np.int32)
    hist = rng.integers(0, 6, (E, max_steps)).astype(np.uint8)
    hist[::7] = 2
    hist[1::9, :8] = np.array([0, 0, 2, 2, 2, 2, 4, 4], np.uint8)  # variance exactly 2.0
    length[1::9] = 8
    success = (rng.random(E) < 0.3).astype(np.uint8)
    contacts = hist[np.arange(E), length - 1].copy()
    return dict(length=length, success=success, contacts=contacts, ret=rng.normal(-3.0, 25.0, E), hist=hist)
