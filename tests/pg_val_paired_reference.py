"""NumPy restatement of the paired validation row (include/dxrl.h, dxrl_pg_val_paired_row): for
level l, pair i is (record l G K + i, record i) of the level-major records; the integer columns
by counting, the moments of the return difference d as (count, mean, M2) triples of d - d_0 per
1,024-pair chunk merged in chunk order with Chan's update, and the three columns derived from
lost / gained by the header's f64 operations in its order.  `two_pass` is the direct reference
the bounds are read against."""
import numpy as np

PAIRED_COLUMNS = ("pairs", "lost", "gained", "both_success", "both_fail", "mean_return_diff", "return_diff_std",
                  "return_diff_stderr", "mean_length_diff", "paired_degradation", "paired_degradation_stderr", "mcnemar",
                  "objects_with_loss", "max_object_lost")
PAIRED_COLS = 14
PIDX = {name: k for k, name in enumerate(PAIRED_COLUMNS)}
INTEGER_COLUMNS = ("pairs", "lost", "gained", "both_success", "both_fail", "objects_with_loss", "max_object_lost")
DERIVED_COLUMNS = ("paired_degradation", "paired_degradation_stderr", "mcnemar")
CHUNK = 1024
NAN = float("nan")


def merge(a, b):
    """Chan et al.'s update of two (n, mean, M2) triples."""
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n = a[0] + b[0]
    d = b[1] - a[1]
    return (n, a[1] + d * (b[0] / n), a[2] + b[2] + d * d * (a[0] * b[0] / n))


def diff_moments(d):
    """(n, mean, M2) of d: chunks of d - d[0] merged in order; the mean carries d[0] back."""
    d = np.asarray(d, dtype=np.float64)
    x = d - d[0]
    m = (0.0, 0.0, 0.0)
    for i in range(0, x.size, CHUNK):
        c = x[i:i + CHUNK]
        mean = float(c.mean())
        m = merge(m, (float(c.size), mean, float(((c - mean) ** 2).sum())))
    return m[0], float(d[0]) + m[1], m[2]


def derived(lost, gained, n):
    """paired_degradation, its standard error and McNemar's statistic: include/dxrl.h's f64
    operations in its order."""
    dn, dc, N = np.float64(lost) - np.float64(gained), np.float64(lost) + np.float64(gained), np.float64(n)
    q = dn * dn
    q = q / N
    v = dc - q
    v = v / N
    v = v if v > 0.0 else np.float64(0.0)
    return {"paired_degradation": float(dn / N), "paired_degradation_stderr": float(np.sqrt(v) / np.sqrt(N)),
            "mcnemar": float((dn * dn) / dc) if dc > 0.0 else 0.0}


def object_lost(G, K, suc0, suc1):
    return ((np.asarray(suc0) != 0) & (np.asarray(suc1) == 0)).reshape(G, K).sum(axis=1).astype(np.int32)


def level_values(G, K, ret0, ret1, len0, len1, suc0, suc1):
    """The paired columns of one level against the baseline, and its per-object lost counts."""
    n = G * K
    s0, s1 = np.asarray(suc0) != 0, np.asarray(suc1) != 0
    lost, gained, both = int((s0 & ~s1).sum()), int((~s0 & s1).sum()), int((s0 & s1).sum())
    d = np.asarray(ret1, dtype=np.float64) - np.asarray(ret0, dtype=np.float64)
    cnt, mean, m2 = diff_moments(d)
    dlen = int(np.asarray(len1, dtype=np.int64).sum() - np.asarray(len0, dtype=np.int64).sum())
    per_object = object_lost(G, K, suc0, suc1)
    r = {"pairs": float(n), "lost": float(lost), "gained": float(gained), "both_success": float(both),
         "both_fail": float(n - lost - gained - both), "mean_return_diff": mean,
         "return_diff_std": float(np.sqrt(m2 / cnt)),
         "return_diff_stderr": float(np.sqrt(m2 / (cnt * (cnt - 1.0)))) if n > 1 else NAN,
         "mean_length_diff": dlen / float(n), "objects_with_loss": float((per_object > 0).sum()),
         "max_object_lost": float(per_object.max())}
    r.update(derived(lost, gained, n))
    return r, per_object


def paired_row(L, G, K, ep_return, ep_length, ep_success):
    """(list of L column dicts, object_lost i32 [L][G]) of level-major records."""
    n = G * K
    ret, length, suc = np.asarray(ep_return), np.asarray(ep_length), np.asarray(ep_success)
    rows, objects = [], []
    for l in range(L):
        s = slice(l * n, (l + 1) * n)
        r, o = level_values(G, K, ret[:n], ret[s], length[:n], length[s], suc[:n], suc[s])
        rows.append(r)
        objects.append(o)
    return rows, np.stack(objects)


def paired_array(rows):
    return np.array([[r[name] for name in PAIRED_COLUMNS] for r in rows], dtype=np.float64)


def two_pass(ret0, ret1):
    """(mean, std, stderr) of d = ret1 - ret0 by the direct two-pass f64 reduction."""
    d = np.asarray(ret1, dtype=np.float64) - np.asarray(ret0, dtype=np.float64)
    n = d.size
    mean = float(d.mean())
    m2 = float(((d - mean) ** 2).sum())
    return mean, float(np.sqrt(m2 / n)), float(np.sqrt(m2 / (n * (n - 1.0)))) if n > 1 else NAN


def sum_bound(x):
    """An f64 sum of k terms differs from any other summation order's by at most k 2^-52 sum|x|
    (test_gpu_pg_val.py's bound)."""
    x = np.asarray(x, dtype=np.float64)
    return x.size * 2.0 ** -52 * float(np.abs(x).sum())


SHAPES = [(2, 1, 1), (2, 3, 5), (3, 37, 33), (16, 4, 8), (2, 67, 1001)]
KINDS = ["random", "all_pairs_equal", "offset_returns", "every_success_lost", "no_discordant_pair"]


def records(L, G, K, kind="random", seed=0):
    """Level-major records of a kind: random levels; every level a copy of the baseline; returns
    near 1e6 whose differences are near 1e-3; a baseline with successes and levels without; the
    baseline's successes at every level."""
    rng = np.random.default_rng(seed)
    n = G * K
    E = L * n
    ret = 1.0 + 3.0 * rng.standard_normal(E)
    length = rng.integers(1, 201, E).astype(np.int32)
    suc = ((rng.random(E) < 0.5) * rng.choice([1, 255], E)).astype(np.uint8)
    if kind == "all_pairs_equal":
        ret, length, suc = np.tile(ret[:n], L), np.tile(length[:n], L), np.tile(suc[:n], L)
    elif kind == "offset_returns":
        base = 1e6 + rng.standard_normal(n)
        ret = np.concatenate([base + (1e-3 * l) * (1.0 + 0.1 * rng.standard_normal(n)) for l in range(L)])
    elif kind == "every_success_lost":
        suc[0] = 1  # at least one success to lose
        suc[n:] = 0
    elif kind == "no_discordant_pair":
        suc = np.tile(suc[:n], L)
        nz = suc != 0
        suc[nz] = rng.choice([1, 255], int(nz.sum())).astype(np.uint8)  # other bytes, the same flags
    return dict(L=L, G=G, K=K, ep_return=ret, ep_length=length, ep_success=suc)
