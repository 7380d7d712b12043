"""NumPy / plain-Python restatement of ``dxrl_pg_val_failure_row`` (csrc/dxrl_pg_val_failure.hip)
and the crafted level-major records its tests share.

The per-episode verdicts are ``failure_reference.episode_pass`` (``classify_moments``), which
tests/test_failure_stats_host.py pins to the reference's ``FailureClassifier`` golden.  The sums
are Python integers, the columns the f64 expressions of include/dxrl.h in their order, and the
truth of a confidence sum is ``math.fsum``.
"""
import math

import numpy as np

import failure_reference as FR

MODES, CLASSES = 6, 7
MODE_NAMES = FR.MODE_NAMES
CLASS_NAMES = ["success"] + MODE_NAMES
MODE_COLUMNS = ("count", "frequency", "episode_share", "mean_episode_length", "std_episode_length",
                "mean_final_contacts", "mean_confidence", "objects", "max_object_count", "worst_object")
LEVEL_COLUMNS = ("episodes", "failures", "failure_rate", "dominant_mode", "dominant_frequency", "modes_present",
                 "tie_rows", "mean_confidence")
MIDX = {name: k for k, name in enumerate(MODE_COLUMNS)}
LIDX = {name: k for k, name in enumerate(LEVEL_COLUMNS)}
# columns that are integers or correctly rounded quotients / roots of exact integers
EXACT_MODE_COLUMNS = tuple(c for c in MODE_COLUMNS if c != "mean_confidence")
EXACT_LEVEL_COLUMNS = tuple(c for c in LEVEL_COLUMNS if c != "mean_confidence")
DISTRIBUTION_KEYS = ("count", "frequency", "mean_episode_length", "std_episode_length", "mean_final_contacts",
                     "mean_confidence")
EPS = 2.0 ** -52
MAX_EPISODES = 1 << 19
F64 = np.float64


def sum_bound(x):
    """k 2^-52 sum|x|: a bound on the error of any order of summing the k values of x."""
    x = np.asarray(x, dtype=np.float64)
    return x.size * EPS * float(np.abs(x).sum())


def mode_columns(c, F, n, S1, S2, C1, conf_sum, objects, max_count, worst):
    """The ten columns of one (level, mode) from its integers and its confidence sum: the header's
    f64 expressions in their order."""
    out = np.zeros(len(MODE_COLUMNS))
    out[MIDX["count"]] = c
    out[MIDX["frequency"]] = F64(c) / F64(F) if F > 0 else 0.0
    out[MIDX["episode_share"]] = F64(c) / F64(n)
    out[MIDX["objects"]], out[MIDX["max_object_count"]] = objects, max_count
    out[MIDX["worst_object"]] = worst if c > 0 else -1
    if c > 0:
        out[MIDX["mean_episode_length"]] = F64(S1) / F64(c)
        out[MIDX["std_episode_length"]] = math.sqrt(F64(c * S2 - S1 * S1) / F64(c * c))  # the integers exact
        out[MIDX["mean_final_contacts"]] = F64(C1) / F64(c)
        out[MIDX["mean_confidence"]] = F64(conf_sum) / F64(c)
    return out


def level_columns(counts, n, ties, conf_sum):
    """The eight columns of one level from its six mode counts."""
    F = sum(counts)
    top = max(counts)
    out = np.zeros(len(LEVEL_COLUMNS))
    out[LIDX["episodes"]], out[LIDX["failures"]], out[LIDX["failure_rate"]] = n, F, F64(F) / F64(n)
    out[LIDX["dominant_mode"]] = counts.index(top) if F > 0 else -1  # the first mode with the largest count
    out[LIDX["dominant_frequency"]] = F64(top) / F64(F) if F > 0 else 0.0
    out[LIDX["modes_present"]] = sum(c > 0 for c in counts)
    out[LIDX["tie_rows"]] = ties
    out[LIDX["mean_confidence"]] = F64(conf_sum) / F64(F) if F > 0 else 0.0
    return out


def verdicts(length, success, contacts, moments, max_steps, timeout_steps, success_threshold=3):
    """(mode i8, confidence f64, tie bool) of every record: the moments form, n = the length
    clamped to [0, max_steps], tie rows as the exact comparison decides."""
    return FR.episode_pass(length, success, contacts, moments, max_steps, timeout_steps, success_threshold)


def failure_row(L, G, K, length, contacts, verdict, paired=False):
    """One row of the tables on level-major records: dict(modes f64 [L][6][10], levels f64 [L][8],
    transitions i32 [L][7][7] or None, ints [L][6] of (c, S1, S2, C1) Python integers, conf [L][6]
    of (fsum truth, bound of the mean), level_conf [L] likewise, object_counts i64 [L][G][6])."""
    mode, conf, tie = verdict
    n = G * K
    assert len(mode) == L * n and n <= MAX_EPISODES
    modes, levels = np.zeros((L, MODES, len(MODE_COLUMNS))), np.zeros((L, len(LEVEL_COLUMNS)))
    transitions = np.zeros((L, CLASSES, CLASSES), np.int32) if paired else None
    ints, confs, level_conf = [], [], []
    object_counts = np.zeros((L, G, MODES), np.int64)
    for l in range(L):
        sl = slice(l * n, (l + 1) * n)
        md, cf, ln, nc = mode[sl], conf[sl], length[sl], contacts[sl]
        rows = []
        for m in range(MODES):
            sel = np.flatnonzero(md == m)
            lens, cons = [int(x) for x in ln[sel].tolist()], [int(x) for x in nc[sel].tolist()]
            rows.append((len(sel), sum(lens), sum(x * x for x in lens), sum(cons)))
            object_counts[l, :, m] = (md.reshape(G, K) == m).sum(axis=1)
        counts = [r[0] for r in rows]
        F = sum(counts)
        level_confs = []
        for m, (c, S1, S2, C1) in enumerate(rows):
            values = cf[md == m]
            truth = math.fsum(values.tolist())
            per_object = object_counts[l, :, m]
            top = int(per_object.max())
            modes[l, m] = mode_columns(c, F, n, S1, S2, C1, truth, int((per_object > 0).sum()), top,
                                       int(np.argmax(per_object)))  # argmax: the first maximum
            level_confs.append((truth / c if c else 0.0, sum_bound(values) / c if c else 0.0))
        failed = cf[md >= 0]
        levels[l] = level_columns(counts, n, int(tie[sl].sum()), math.fsum(failed.tolist()))
        ints.append(rows)
        confs.append(level_confs)
        level_conf.append((levels[l, LIDX["mean_confidence"]], sum_bound(failed) / F if F else 0.0))
        if paired:
            np.add.at(transitions[l], (mode[:n].astype(np.int64) + 1, md.astype(np.int64) + 1), 1)
    return dict(modes=modes, levels=levels, transitions=transitions, ints=ints, conf=confs, level_conf=level_conf,
                object_counts=object_counts)


def failure_distribution(row, level=0):
    """``ValidationLog.failure_distribution`` on a restated row: keyed by mode name, the modes that
    occurred, ``compute_failure_distribution``'s entries minus the object properties."""
    out = {}
    for m, name in enumerate(MODE_NAMES):
        r = row["modes"][level, m]
        if r[0] > 0:
            out[name] = {k: (int(r[0]) if k == "count" else float(r[MIDX[k]])) for k in DISTRIBUTION_KEYS}
    return out


# ------------------------------------------------------------------ crafted records
MAX_STEPS = 37      # failure_reference.synthetic_records' history pitch, and the timeout bound here
POOL = 512          # rows of the pool; its crafted prefix reaches every rule, mode and both tie kinds
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 8, 12), (16, 2, 3), (2, 256, 264)]
KINDS = ["synthetic", "all_success", "equal_timeouts", "levels_copy", "one_object"]
_pool = {}


def pool():
    """The pool every crafted buffer draws its rows from, with its moments and verdicts: computed
    once and left unchanged."""
    if not _pool:
        d = FR.synthetic_records(POOL, max_steps=MAX_STEPS)
        mom = FR.moments_of(d["hist"], d["length"], MAX_STEPS)
        mode, conf, tie = verdicts(d["length"], d["success"], d["contacts"], mom, MAX_STEPS, MAX_STEPS)
        assert set(mode.tolist()) == set(range(-1, MODES)) and tie.any()
        _pool.update(length=d["length"], success=d["success"], contacts=d["contacts"], moments=mom, mode=mode,
                     conf=conf, tie=tie)
        for v in _pool.values():
            v.setflags(write=False)
    return _pool


def records(L, G, K, kind, seed=0):
    """Level-major records of `kind` as rows of the pool: dict(L, G, K, ep_length i32, ep_success u8,
    ep_contacts u8, hist_moments i32 [E][5], max_steps, timeout_steps, verdict)."""
    p = pool()
    n, E = G * K, L * G * K
    rng = np.random.default_rng(1000 + seed)
    of_mode = {m: np.flatnonzero((p["mode"] == m) & (p["length"] < MAX_STEPS if m != FR.TIMEOUT else True))
               for m in range(-1, MODES)}
    if kind == "synthetic":  # every pool row where E reaches the pool, under a fixed permutation
        idx = np.concatenate([np.arange(POOL), rng.integers(0, POOL, E - POOL)]) if E >= POOL else \
            rng.choice(POOL, E, replace=False)
        idx = idx[rng.permutation(E)]
    elif kind == "all_success":
        idx = rng.choice(of_mode[-1], E)
    elif kind == "equal_timeouts":  # every failure a timeout of the same length
        idx = np.where(rng.random(E) < 0.3, rng.choice(of_mode[-1], E), of_mode[FR.TIMEOUT][0])
        idx[0] = of_mode[FR.TIMEOUT][0]
    elif kind == "levels_copy":
        idx = np.tile(rng.integers(0, POOL, n), L)
    elif kind == "one_object":  # the last object holds every dropped episode, and nothing else
        idx = rng.choice(np.flatnonzero(p["mode"] != FR.DROPPED), E)
        for l in range(L):
            idx[l * n + (G - 1) * K:(l + 1) * n] = rng.choice(of_mode[FR.DROPPED], K)
    else:
        raise ValueError(kind)
    return dict(L=L, G=G, K=K, kind=kind, max_steps=MAX_STEPS, timeout_steps=MAX_STEPS,
                ep_length=p["length"][idx].copy(), ep_success=p["success"][idx].copy(),
                ep_contacts=p["contacts"][idx].copy(), hist_moments=p["moments"][idx].copy(),
                verdict=(p["mode"][idx], p["conf"][idx], p["tie"][idx]))


def hand_written():
    """(1, 1, 1): one episode of 12 steps that held 4 contacts and ended with none -- dropped."""
    hist = np.array([[4] * 12], np.uint8)
    length = np.array([12], np.int32)
    d = dict(L=1, G=1, K=1, kind="hand_written", max_steps=20, timeout_steps=20, ep_length=length,
             ep_success=np.zeros(1, np.uint8), ep_contacts=np.zeros(1, np.uint8),
             hist_moments=FR.moments_of(hist, length, 20))
    d["verdict"] = verdicts(length, d["ep_success"], d["ep_contacts"], d["hist_moments"], 20, 20)
    return d
