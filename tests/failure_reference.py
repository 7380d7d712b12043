"""NumPy / plain-Python restatement of ``dxrl_failure_summarize`` (csrc/dxrl_failure_summary.hip)
and the synthetic record set its tests and tests/golden/gen_failure_golden.py share.

``episode_pass`` is the per-episode launch written one episode at a time in Python integers from
the five history moments (S1, S2, first-five sum, last-five sum, peak), independent of
failures.FailureClassifier, which the golden fixture compares it with.  ``group_pass`` is the
per (group, mode) launch with two-pass f64 moments.  Tie rows -- np.var's own rounding decides a
rule, see include/dxrl.h -- get the exact comparison's answer and a flag; ``settle`` is the host
half of the history form (np.var on those rows only).
"""
import numpy as np

SLIPPAGE, UNSTABLE, MISALIGNMENT, TIMEOUT, DROPPED, INSUFFICIENT = range(6)  # list(FailureMode) order
MODE_NAMES = ["slippage", "unstable_grasp", "misalignment", "timeout", "object_dropped", "insufficient_contacts"]


def moments_of(hist, length, max_steps):
    """i32 [E][5]: S1, S2, F, L, peak of the first min(length, max_steps) entries of each row."""
    E = len(length)
    out = np.zeros((E, 5), np.int32)
    for e in range(E):
        n = max(0, min(int(length[e]), max_steps))
        row = [int(c) for c in hist[e, :n]]
        out[e] = (sum(row), sum(c * c for c in row), sum(row[:5]), sum(row[-5:]) if n else 0, max(row) if n else 0)
    return out


def classify_moments(success, length, n, s1, s2, f5, l5, peak, nc, timeout_steps, success_threshold=3):
    """(mode, confidence, tie) of one episode: the rules of include/dxrl.h in Python integers."""
    if success:
        return -1, 0.0, False
    if n == 0:
        peak = nc
    if length >= timeout_steps:
        return TIMEOUT, 1.0, False
    if nc == 0 and peak > 0:
        return DROPPED, 1.0, False
    num = n * s2 - s1 * s1
    tie = False
    if n > 5:
        if n > 10:
            trend = np.float64(l5) / 5.0 - np.float64(f5) / 5.0
            if trend < -1.0 and peak >= 1:
                return SLIPPAGE, float(min(1.0, abs(trend) / 2.0)), False
        if num > 2 * n * n:
            return UNSTABLE, float(min(1.0, (num / (n * n)) / 5.0)), False  # int / int: correctly rounded
        tie = num == 2 * n * n
    if 1 <= nc <= 2:
        if n <= 1 or num < n * n:
            return MISALIGNMENT, 0.8, tie
        tie = tie or num == n * n
    return INSUFFICIENT, (1.0 if peak < success_threshold else 0.5), tie


def episode_pass(length, success, contacts, moments, max_steps, timeout_steps, success_threshold=3):
    E = len(length)
    mode, conf, tie = np.full(E, -1, np.int8), np.zeros(E), np.zeros(E, bool)
    for e in range(E):
        n = max(0, min(int(length[e]), max_steps))
        s1, s2, f5, l5, pk = (int(x) for x in moments[e])
        mode[e], conf[e], tie[e] = classify_moments(bool(success[e]), int(length[e]), n, s1, s2, f5, l5, pk,
                                                    int(contacts[e]), timeout_steps, success_threshold)
    return mode, conf, tie


def settle(mode, conf, tie, length, contacts, hist, success_threshold=3):
    """What np.var decides on the tie rows (they are past the timeout, dropped and slippage
    rules): returns copies of ``mode`` / ``conf`` with those rows re-decided."""
    mode, conf = mode.copy(), conf.copy()
    for e in np.flatnonzero(tie):
        n, nc = int(length[e]), int(contacts[e])
        counts = [int(c) for c in hist[e, :n]]
        var = np.var(counts) if n > 1 else 0.0
        if n > 5 and var > 2.0:
            mode[e], conf[e] = UNSTABLE, min(1.0, var / 5.0)
        elif 1 <= nc <= 2 and var < 1.0:
            mode[e], conf[e] = MISALIGNMENT, 0.8
        else:
            mode[e], conf[e] = INSUFFICIENT, (1.0 if max(counts) < success_threshold else 0.5)
    return mode, conf


def group_pass(mode, skip, tie, length, success, contacts, props, groups):
    """mode_stats i64 [G][6][8], group_totals i64 [G][4], mode_props f64 [G][6][3][5] (two-pass
    mean and M2); episodes with ``skip`` set stay out of the mode tables."""
    G = len(groups)
    stats, totals, mp = np.zeros((G, 6, 8), np.int64), np.zeros((G, 4), np.int64), np.zeros((G, 6, 3, 5))
    for g, idx in enumerate(groups):
        idx = np.asarray(idx, dtype=np.int64)
        if not len(idx):
            continue
        totals[g, :3] = len(idx), success[idx].astype(bool).sum(), tie[idx].sum()
        for k in range(6):
            sel = idx[(mode[idx] == k) & ~skip[idx]]
            if not len(sel):
                continue
            n, c = length[sel].astype(np.int64), contacts[sel].astype(np.int64)
            stats[g, k, :5] = len(sel), n.sum(), (n * n).sum(), c.sum(), (c * c).sum()
            for q in range(3):
                x = props[sel, q].astype(np.float64)
                mp[g, k, q] = len(sel), np.mean(x), np.sum((x - np.mean(x)) ** 2), x.min(), x.max()
    return stats, totals, mp


# ------------------------------------------------------------------ synthetic records
def _tie_rows(kind, want_each=1, seed=2024, max_n=30):
    """Count rows on a tie of the variance rules with a non-integer mean (searched), on either
    side of np.var's rounding: kind 2 -> n^2 var == 2 n^2 (np.var > 2.0 or not), kind 1 ->
    n^2 var == n^2 (np.var < 1.0 or not)."""
    rng = np.random.default_rng(seed + kind)
    moved, kept = [], []
    for _ in range(400000):
        if len(moved) >= want_each and len(kept) >= want_each:
            break
        n = int(rng.integers(6, max_n))
        c = rng.integers(0, 6, n) if kind == 2 else rng.integers(0, 4, n)
        if n * int((c * c).sum()) - int(c.sum()) ** 2 != kind * n * n or int(c.sum()) % n == 0:
            continue
        v = np.var(c.astype(np.int64))
        (moved if (v > 2.0 if kind == 2 else v < 1.0) else kept).append(c.tolist())
    assert moved and kept, f"no tie rows of kind {kind} on both sides of np.var's rounding"
    return moved[:want_each] + kept[:want_each]


def _random_history(rng, n, dist):
    if dist == 0:
        return rng.integers(0, 6, n)                                   # uniform counts
    if dist == 1:
        return rng.choice(3, n, p=[0.5, 0.35, 0.15])                   # few contacts
    if dist == 2:                                                      # contacts made, then lost
        return np.clip(np.round(np.linspace(4.5, 0.5, n) + rng.normal(0, 0.8, n)), 0, 5).astype(np.int64)
    return rng.choice([0, 1, 4, 5], n, p=[0.35, 0.15, 0.15, 0.35])     # jumping counts


def synthetic_records(E, max_steps=37, seed=11):
    """Records that reach every rule, every mode and both tie kinds; the crafted rows come first
    and the random ones are drawn one after the other, so a smaller E is a prefix of a larger.
    Returns dict(length i32, success u8, contacts u8, props f64 [E][3], hist u8 [E][max_steps])."""
    rng = np.random.default_rng(seed)
    rows = []  # (history, success, contacts)

    def add(h, success=0, contacts=None):
        h = [int(c) for c in h]
        rows.append((h, success, h[-1] if contacts is None else contacts))

    for n in (1, 5, 6, 10, 11, max_steps):
        add([2] * n, contacts=3)                       # constant, peak < 3: insufficient 1.0
        add([3] * n, contacts=3)                       # peak >= 3: insufficient 0.5
        add([1] * n, success=1, contacts=4)            # success
        add([3] * n, contacts=0)                       # dropped
        add([0] * n, contacts=0)                       # never touched: not dropped
        for nc in (1, 2):
            add([nc] * n, contacts=nc)                 # misalignment
        add([5] * (n - n // 2) + [0] * (n // 2), contacts=1)   # falling: slippage (n > 10) or unstable
        add(([0, 5] * n)[:n], contacts=2)              # jumping: unstable (n > 5)
        for _ in range(3):
            add(rng.integers(0, 6, n), success=int(rng.random() < 0.3), contacts=int(rng.integers(0, 6)))
    add([4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 3], contacts=3)  # trend exactly -1.0: not slippage
    add([5, 5, 5, 5, 5, 2, 1, 1, 1, 1, 1, 1], contacts=1)  # |trend| / 2 > 1: confidence clamps
    for h in [[0, 0, 0, 0, 3, 3], [3, 3, 0, 0, 0, 0, 0, 0, 3]] + _tie_rows(2):
        add(h, contacts=3)                             # tie of rule 4
    add([0, 0, 0, 0, 3, 3], success=1, contacts=3)     # closed before the tie: no tie row
    add([0, 0, 0, 0, 3, 4], contacts=3)                # just above / below
    add([0, 0, 0, 1, 3, 3], contacts=3)
    for h in [[0, 2], [0, 0, 2, 2], [2, 0, 2, 0, 2, 0]] + _tie_rows(1):
        add(h, contacts=2)                             # tie of rule 5 (n = 2, 4: no unstable rule)
        add(h, contacts=3)                             # same row, rule 5 closed: no tie
    add([1, 0, 2, 0, 2, 1], contacts=1)
    crafted = len(rows)
    assert E >= crafted, f"E must be at least {crafted}"
    for i in range(E - crafted):                       # random histories of every length
        n = 1 + i % max_steps
        h = _random_history(rng, n, (i // max_steps) % 4)
        add(h, success=int(rng.random() < 0.15), contacts=int(h[-1]) if rng.random() < 0.8 else int(rng.integers(0, 6)))
    fill = np.random.default_rng(seed + 1)
    hist = fill.integers(0, 256, (E, max_steps)).astype(np.uint8)  # garbage past each row's length
    length = np.zeros(E, np.int32)
    for e, (h, _, _) in enumerate(rows):
        length[e] = len(h)
        hist[e, :len(h)] = h
    props = np.stack([fill.uniform(0.03, 0.1, E), fill.uniform(0.05, 0.3, E), fill.uniform(0.2, 0.9, E)], 1)
    return dict(length=length, success=np.array([r[1] for r in rows], np.uint8),
                contacts=np.array([r[2] for r in rows], np.uint8), props=props, hist=hist)


def episode_dicts(d, idx=None):
    """The records as the episode dictionaries FailureClassifier reads (with the logged form's
    ``object_properties``)."""
    out = []
    for e in (range(len(d["length"])) if idx is None else idx):
        n = int(d["length"][e])
        out.append({"success": bool(d["success"][e]), "episode_steps": n, "num_contacts": int(d["contacts"][e]),
                    "final_contacts": int(d["contacts"][e]),
                    "contact_history": [[1.0 if j < c else 0.0 for j in range(5)] for c in d["hist"][e, :n].tolist()],
                    "object_properties": {"size": float(d["props"][e, 0]), "mass": float(d["props"][e, 1]),
                                          "friction_coefficient": float(d["props"][e, 2])}})
    return out
