"""NumPy restatement of dxrl_study_summarize (csrc/dxrl_study_summary.hip) in the kernel's own
operation order: episode e on wave lane e % 64 with a Welford step per episode and Chan's merge
in the shuffle tree, the left-to-right moving average and its tie band, and the group pass's
member-to-thread assignment and LDS tree.  Every f64 operation is an IEEE operation in the same
order as on the device, so the GPU tests compare the f64 columns bit for bit."""
import numpy as np

WAVE, GROUP_THREADS = 64, 128
LANE_INTS, LANE_REALS, METRICS = 8, 4, 5
EPISODES, STEPS, SUCCESSES, FINAL_WINDOW, CONV, REWARD_CONV, LEVEL, FLAGS = range(8)
FLAG_TIE, FLAG_SKIPPED = 1, 2
ST_RANGE, ST_TIE_CAP, ST_LANE, ST_MIXED = 1, 2, 4, 8
EPS64 = np.float64(2.0) ** -46  # 64 eps

f64 = np.float64


def merge(a, b):
    """Chan et al.'s pairwise update on (n, mean, M2)."""
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n = a[0] + b[0]
    d = b[1] - a[1]
    return (n, a[1] + d * (b[0] / n), a[2] + b[2] + d * d * (a[0] * b[0] / n))


def push(m, x):
    n1 = m[0] + f64(1.0)
    d = x - m[1]
    mean = m[1] + d / n1
    return (n1, mean, m[2] + d * (x - mean))


ZERO = (f64(0.0), f64(0.0), f64(0.0))


def tree(parts):
    """for s = T/2 .. 1: part[t] = merge(part[t], part[t + s]) for t < s."""
    parts = list(parts)
    s = len(parts) // 2
    while s >= 1:
        for t in range(s):
            parts[t] = merge(parts[t], parts[t + s])
        s //= 2
    return parts[0]


def moving_average(r, w):
    """ma_i and the tie band of every window, left to right."""
    inv = f64(1.0) / f64(w)
    n = len(r) - w + 1
    ma, band = np.zeros(n), np.zeros(n)
    for i in range(n):
        a, mx = f64(0.0), f64(0.0)
        for j in range(w):
            p = r[i + j] * inv
            a = a + p
            mx = max(mx, abs(p))
        ma[i], band[i] = a, (mx * f64(w)) * EPS64
    return ma, band


def lane_row(r, steps, success, level, w, c_min, thr):
    """One lane's (ints, reals) from its E records."""
    with np.errstate(all="ignore"):
        r = np.asarray(r, dtype=np.float64)
        ok = np.asarray(success).astype(bool)
        E = len(r)
        K = r[0]
        parts = [ZERO] * WAVE
        for e in range(E):
            parts[e % WAVE] = push(parts[e % WAVE], r[e] - K)
        mo = tree(parts)
        conv = -1
        for i in range(w, E):
            if int(ok[i - w:i].sum()) >= c_min:
                conv = i
                break
        rconv, tie = -1, False
        if E >= w:
            ma, band = moving_average(r, w)
            cross = np.flatnonzero(ma >= thr)
            near = np.flatnonzero(np.abs(ma - f64(thr)) <= band)
            if len(cross):
                rconv = int(cross[0]) + w - 1
            tie = bool(len(near)) and (not len(cross) or near[0] <= cross[0])
        else:
            cross = np.flatnonzero(r >= thr)
            if len(cross):
                rconv = int(cross[0]) + w - 1
        k = min(w, E)
        fsum = f64(0.0)
        for e in range(E - k, E):
            fsum = fsum + r[e]
        ints = np.array([E, int(np.asarray(steps, dtype=np.int64).sum()), int(ok.sum()), int(ok[E - k:].sum()), conv,
                         rconv, -1 if level is None else int(level[E - 1]), FLAG_TIE if tie else 0], dtype=np.int64)
        reals = np.array([mo[0], K + mo[1], mo[2], fsum / f64(k)], dtype=np.float64)
    return ints, reals


def lane_pass(ep_return, ep_length, ep_success, ep_level, lane_episodes, w, c_min, thr, lane_ints=None,
              lane_reals=None, lane_offset=0):
    """Rows lane_offset .. lane_offset + N of the lane table; returns (lane_ints, lane_reals, status)."""
    n = len(lane_episodes)
    cap = np.asarray(ep_return).shape[1]
    if lane_ints is None:
        lane_ints = np.zeros((lane_offset + n, LANE_INTS), dtype=np.int64)
        lane_reals = np.zeros((lane_offset + n, LANE_REALS), dtype=np.float64)
    status = 0
    for l in range(n):
        E = int(lane_episodes[l])
        row = lane_offset + l
        if E <= 0 or E > cap:
            lane_ints[row] = [0, 0, 0, 0, -1, -1, -1, FLAG_SKIPPED]
            lane_reals[row] = 0.0
            status |= ST_LANE
            continue
        lane_ints[row], lane_reals[row] = lane_row(ep_return[l][:E], ep_length[l][:E], ep_success[l][:E],
                                                   None if ep_level is None else ep_level[l], w, c_min, thr)
    return lane_ints, lane_reals, status


def lane_metrics(reals):
    """(values, CV finite) of one lane: variance, std, CV, final reward, mean reward."""
    with np.errstate(all="ignore"):
        var = f64(reals[2]) / f64(reals[0])
        sd = np.sqrt(var)
        mean = f64(reals[1])
        fin = bool(mean != 0.0)
        return [var, sd, sd / mean if fin else f64(0.0), f64(reals[3]), mean], fin


def group_pass(lane_ints, lane_reals, group_offsets, group_lanes, tie_cap, num_members=None):
    """(group_stats i64 [G][16], group_metrics f64 [G][5][3], tie_list, tie_count, status)."""
    L = len(lane_ints)
    G = len(group_offsets) - 1
    num_members = len(group_lanes) if num_members is None else num_members
    stats = np.zeros((G, 16), dtype=np.int64)
    metrics = np.zeros((G, METRICS, 3), dtype=np.float64)
    status = 0
    T = GROUP_THREADS
    with np.errstate(all="ignore"):
        for g in range(G):
            lo, hi = int(group_offsets[g]), int(group_offsets[g + 1])
            bad = lo < 0 or hi < lo or hi > num_members
            K = [f64(0.0)] * METRICS
            if not bad and lo < hi:
                l0 = int(group_lanes[lo])
                if 0 <= l0 < L and lane_ints[l0][EPISODES] > 0:
                    K, _ = lane_metrics(lane_reals[l0])
            acc = np.zeros(16, dtype=object)
            fw_all, e_all = [], []
            parts = [[ZERO] * T for _ in range(METRICS)]
            if not bad:
                for m in range(lo, hi):
                    l = int(group_lanes[m])
                    if l < 0 or l >= L:
                        bad = True
                        continue
                    li = [int(x) for x in lane_ints[l]]
                    if li[EPISODES] <= 0:
                        continue
                    t = (m - lo) % T
                    acc[0] += 1
                    acc[1] += li[EPISODES]
                    acc[2] += li[STEPS]
                    acc[3] += li[STEPS] ** 2
                    acc[4] += li[FINAL_WINDOW]
                    acc[5] += li[FINAL_WINDOW] ** 2
                    fw_all.append(li[FINAL_WINDOW])
                    e_all.append(li[EPISODES])
                    if li[CONV] >= 0:
                        acc[8] += 1
                        acc[9] += li[CONV]
                        acc[10] += li[CONV] ** 2
                    if li[REWARD_CONV] >= 0:
                        acc[11] += 1
                        acc[12] += li[REWARD_CONV]
                        acc[13] += li[REWARD_CONV] ** 2
                    acc[14] += 1 if li[FLAGS] & FLAG_TIE else 0
                    acc[15] += li[SUCCESSES]
                    v, fin = lane_metrics(lane_reals[l])
                    for k in range(METRICS):
                        if k != 2 or fin:
                            parts[k][t] = push(parts[k][t], v[k] - K[k])
            if bad:
                status |= ST_RANGE
            if fw_all:
                acc[6], acc[7] = min(fw_all), max(fw_all)
                if min(e_all) != max(e_all):
                    status |= ST_MIXED
            stats[g] = [int(x) for x in acc]
            for k in range(METRICS):
                mo = tree(parts[k])
                metrics[g, k] = [mo[0], K[k] + mo[1] if mo[0] > 0.0 else mo[1], mo[2]]
    ties = [l for l in range(L) if lane_ints[l][FLAGS] & FLAG_TIE]
    if len(ties) > tie_cap:
        status |= ST_TIE_CAP
    return stats, metrics, ties[:tie_cap], len(ties), status
