"""NumPy restatement of the rank record and the rank-order merge of the sharded training log
(include/dxrl.h, dxrl_pg_log_rank_pack / dxrl_pg_log_row_world).  A record holds plain f64 sums and
two-pass (mean, M2) pairs -- the definitions, not the device's summation order; the merge is the
device's: f64 additions and Chan's update, in rank order."""
import math

import numpy as np

import pg_log_reference as L

RANK_COLUMNS = ("samples", "reward_sum", "value_sum", "done_count", "target_mean", "target_m2", "residual_mean",
                "residual_m2", "episodes", "length_sum", "successes", "return_sum", "policy_loss_sum",
                "value_se_sum", "clip_sum", "kl_sum", "loss_rows")
RANK_DOUBLES = 20
R = {name: k for k, name in enumerate(RANK_COLUMNS)}


EPS = 2.0 ** -52
EXACT = ("iteration", "env_steps", "episodes", "mean_length", "success_rate", "done_fraction", "adv_mean", "adv_std")
LOSS = ("policy_loss", "value_mse", "clip_frac", "approx_kl")


def sum_bound(x):
    """k 2^-52 sum|x|: two f64 sums of the same k terms, in any two orders, differ by at most this
    (tests/test_gpu_pg_log.py derives it)."""
    x = np.asarray(x, dtype=np.float64)
    return x.size * EPS * float(np.abs(x).sum())


def assert_row_within_bounds(got, ref, ep_sum_return, rew, ret, values, loss_partial, loss_rows, what=""):
    """`got` (column -> value) against `ref` (row_values on the concatenated arrays, which are the
    other arguments: values already cut to the samples): integer-derived columns exact, f64 sums
    within sum_bound / count, variances and explained_variance within 1e-9 relative."""
    for name in EXACT:
        assert got[name] == ref[name], (what, name, got[name], ref[name])
    M, eps_n = np.asarray(rew).size, ref["episodes"]
    for name, terms, count in (("mean_return", ep_sum_return, eps_n), ("mean_step_reward", rew, M),
                               ("value_mean", values, M), ("target_mean", ret, M)):
        if count == 0:
            assert math.isnan(got[name]) and math.isnan(ref[name]), (what, name)
            continue
        bound = sum_bound(terms) / count
        print(what, name, got[name], ref[name], abs(got[name] - ref[name]), bound)
        assert abs(got[name] - ref[name]) <= bound, (what, name)
    loss = np.asarray(loss_partial, dtype=np.float64).reshape(-1, 4)
    for k, name in enumerate(LOSS):
        bound = sum_bound(loss[:, k]) / loss_rows
        print(what, name, got[name], ref[name], abs(got[name] - ref[name]), bound)
        assert abs(got[name] - ref[name]) <= bound, (what, name)
    assert abs(got["grad_norm"] - ref["grad_norm"]) <= EPS * ref["grad_norm"], what  # one rounding of sqrt
    for name in ("target_var", "residual_var", "explained_variance"):
        print(what, name, got[name], ref[name], abs(got[name] / ref[name] - 1.0))
        assert abs(got[name] - ref[name]) <= 1e-9 * abs(ref[name]), (what, name)


def shard_inputs(n, T, seed, episodes=True, blocks=5):
    """Host arrays of one rank's iteration (logical sizes; tests/test_gpu_pg_log.py's `inputs`
    with a per-rank seed).  ret: mean 5, std 1, so |mean| / std <= 10; values = ret + noise, with
    the n bootstrap entries behind the samples.  episodes=False: a rank that finished none."""
    rng = np.random.default_rng(seed)
    M = n * T
    ret = (5.0 + rng.standard_normal(M)).astype(np.float32)
    values = np.concatenate([ret + 0.5 * rng.standard_normal(M).astype(np.float32),
                             rng.standard_normal(n).astype(np.float32)]).astype(np.float32)
    d = dict(n=n, T=T, ep_count=rng.integers(0, 4, n).astype(np.int32), ep_sum_return=rng.standard_normal(n) * 3,
             ep_sum_length=rng.integers(0, 90, n).astype(np.int32), ep_successes=rng.integers(0, 3, n).astype(np.int32),
             rew=rng.standard_normal(M).astype(np.float32), ret=ret, done=(rng.random(M) < 0.1).astype(np.uint8) * 3,
             values=values, loss_partial=rng.standard_normal((blocks, 4)), loss_rows=M // 2)
    if not episodes:
        d["ep_count"][:] = 0
        d["ep_sum_return"][:] = 0.0
        d["ep_sum_length"][:] = 0
        d["ep_successes"][:] = 0
    return d


def concatenated(shards):
    """The arguments of row_values for the batch of all shards (samples cut to each rank's n * T;
    any order of the samples gives the same definitions)."""
    cat = lambda k, cut=False: np.concatenate(  # noqa: E731
        [np.asarray(d[k])[:d["n"] * d["T"]] if cut else np.asarray(d[k]) for d in shards])
    T = shards[0]["T"]
    assert all(d["T"] == T for d in shards)
    return dict(n=sum(d["n"] for d in shards), T=T, ep_count=cat("ep_count"), ep_sum_return=cat("ep_sum_return"),
                ep_sum_length=cat("ep_sum_length"), ep_successes=cat("ep_successes"), rew=cat("rew", True),
                ret=cat("ret", True), done=cat("done", True), values=cat("values", True),
                loss_partial=np.concatenate([np.asarray(d["loss_partial"]).reshape(-1, 4) for d in shards]),
                loss_rows=sum(d["loss_rows"] for d in shards))


def record_of(d):
    return rank_record(d["n"], d["T"], d["ep_count"], d["ep_sum_return"], d["ep_sum_length"], d["ep_successes"],
                       d["rew"], d["ret"], d["done"], d["values"], d["loss_partial"], d["loss_rows"])


def mean_m2(x):
    x = np.asarray(x, dtype=np.float64)
    m = float(x.mean())
    return m, float(((x - m) ** 2).sum())


def rank_record(n, T, ep_count, ep_sum_return, ep_sum_length, ep_successes, rew, ret, done, values, loss_partial,
                loss_rows):
    """One rank's record from its own arrays (only the first n * T samples are read)."""
    M = n * T
    rew, ret, val = (np.asarray(x, dtype=np.float64)[:M] for x in (rew, ret, values))
    rec = np.zeros(RANK_DOUBLES)
    rec[R["samples"]] = M
    rec[R["reward_sum"]], rec[R["value_sum"]] = rew.sum(), val.sum()
    rec[R["done_count"]] = np.count_nonzero(np.asarray(done)[:M])
    rec[R["target_mean"]], rec[R["target_m2"]] = mean_m2(ret)
    rec[R["residual_mean"]], rec[R["residual_m2"]] = mean_m2(ret - val)
    rec[R["episodes"]] = int(np.asarray(ep_count, dtype=np.int64)[:n].sum())
    rec[R["length_sum"]] = int(np.asarray(ep_sum_length, dtype=np.int64)[:n].sum())
    rec[R["successes"]] = int(np.asarray(ep_successes, dtype=np.int64)[:n].sum())
    rec[R["return_sum"]] = np.asarray(ep_sum_return, dtype=np.float64)[:n].sum()
    rec[R["policy_loss_sum"]:R["kl_sum"] + 1] = np.asarray(loss_partial, dtype=np.float64).reshape(-1, 4).sum(0)
    rec[R["loss_rows"]] = loss_rows
    return rec


def merge(a, b):
    """Chan's update of (n, mean, M2) triples (csrc/dxrl_moments.h merge)."""
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n = a[0] + b[0]
    d = b[1] - a[1]
    return (n, a[1] + d * (b[0] / n), a[2] + b[2] + d * d * (a[0] * b[0] / n))


def merged_values(records, iteration, env_steps, stats, gnorm2):
    """The columns before is_best of the row finished from `records` ([world][RANK_DOUBLES]) in
    rank order, as pg_log_reference.row_values returns them."""
    records = np.asarray(records, dtype=np.float64).reshape(-1, RANK_DOUBLES)
    s = {name: 0.0 for name in RANK_COLUMNS}
    mt = mr = (0.0, 0.0, 0.0)
    for rec in records:
        for name in RANK_COLUMNS:
            s[name] = s[name] + float(rec[R[name]])
        n = float(rec[R["samples"]])
        mt = merge(mt, (n, float(rec[R["target_mean"]]), float(rec[R["target_m2"]])))
        mr = merge(mr, (n, float(rec[R["residual_mean"]]), float(rec[R["residual_m2"]])))
    M, eps = mt[0], s["episodes"]
    out = {"iteration": float(iteration), "env_steps": float(env_steps), "episodes": eps}
    for name, key in (("mean_return", "return_sum"), ("mean_length", "length_sum"), ("success_rate", "successes")):
        out[name] = s[key] / eps if eps > 0.0 else L.NAN
    out["mean_step_reward"], out["done_fraction"], out["value_mean"] = s["reward_sum"] / M, s["done_count"] / M, \
        s["value_sum"] / M
    tvar, rvar = mt[2] / mt[0], mr[2] / mr[0]
    out["target_mean"], out["target_var"], out["residual_var"] = mt[1], tvar, rvar
    out["explained_variance"] = L.NAN if tvar == 0.0 else 1.0 - rvar / tvar
    stats = np.asarray(stats, dtype=np.float64)
    out["adv_mean"], out["adv_std"] = float(stats[2]), float(stats[4])
    for name, key in (("policy_loss", "policy_loss_sum"), ("value_mse", "value_se_sum"), ("clip_frac", "clip_sum"),
                      ("approx_kl", "kl_sum")):
        out[name] = s[key] / s["loss_rows"]
    out["grad_norm"] = math.sqrt(float(gnorm2))
    return out
