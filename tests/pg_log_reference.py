"""NumPy restatement of the training-log row, header and window rules (include/dxrl.h,
dxrl_pg_log_row).  Sums are plain f64 sums, variances two-pass f64 -- the definitions, not the
device's summation order."""
import math

import numpy as np

COLUMNS = ("iteration", "env_steps", "episodes", "mean_return", "mean_length", "success_rate",
           "mean_step_reward", "done_fraction", "value_mean", "target_mean", "target_var", "residual_var",
           "explained_variance", "adv_mean", "adv_std", "policy_loss", "value_mse", "clip_frac", "approx_kl",
           "grad_norm", "is_best", "window_mean")
COLS = 24
IDX = {name: k for k, name in enumerate(COLUMNS)}
IS_BEST = IDX["is_best"]
NAN = float("nan")


def new_header():
    return {"rows_written": 0, "best_row": -1, "converged_row": -1, "best_score": -math.inf}


def two_pass_var(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.mean((x - x.mean()) ** 2))


def row_values(n, T, iteration, env_steps, ep_count, ep_sum_return, ep_sum_length, ep_successes, rew, ret, done,
               values, stats, loss_partial, loss_rows, gnorm2):
    """Columns before is_best, as a dict.  Only the first n * T entries of the sample buffers are
    read (values carries n more: the bootstrap slot)."""
    M = n * T
    rew, ret, val = (np.asarray(x, dtype=np.float64)[:M] for x in (rew, ret, values))
    done = np.asarray(done)[:M]
    episodes = int(np.asarray(ep_count, dtype=np.int64)[:n].sum())
    out = {"iteration": float(iteration), "env_steps": float(env_steps), "episodes": float(episodes)}
    if episodes:
        out["mean_return"] = float(np.asarray(ep_sum_return, dtype=np.float64)[:n].sum()) / episodes
        out["mean_length"] = int(np.asarray(ep_sum_length, dtype=np.int64)[:n].sum()) / episodes
        out["success_rate"] = int(np.asarray(ep_successes, dtype=np.int64)[:n].sum()) / episodes
    else:
        out["mean_return"] = out["mean_length"] = out["success_rate"] = NAN
    out["mean_step_reward"] = float(rew.sum()) / M
    out["done_fraction"] = int(np.count_nonzero(done)) / M
    out["value_mean"] = float(val.sum()) / M
    out["target_mean"] = float(ret.mean())
    out["target_var"] = two_pass_var(ret)
    out["residual_var"] = two_pass_var(ret - val)
    out["explained_variance"] = NAN if out["target_var"] == 0.0 else 1.0 - out["residual_var"] / out["target_var"]
    stats = np.asarray(stats, dtype=np.float64)
    out["adv_mean"], out["adv_std"] = float(stats[2]), float(stats[4])
    loss = np.asarray(loss_partial, dtype=np.float64).reshape(-1, 4).sum(0) / loss_rows
    for k, name in enumerate(("policy_loss", "value_mse", "clip_frac", "approx_kl")):
        out[name] = float(loss[k])
    out["grad_norm"] = math.sqrt(float(gnorm2))
    return out


def finish_row(table, header, row, values, score_col=-1, min_episodes=1, conv_col=-1, window=1, threshold=0.0):
    """Write `values` (row_values' dict) as table[row] and apply keep-best and convergence to
    `header` in place.  Returns the is_best flag."""
    out = np.zeros(COLS)
    for name, v in values.items():
        out[IDX[name]] = v
    best = False
    if score_col >= 0:
        score = out[score_col]
        if values["episodes"] >= min_episodes and score > header["best_score"]:  # NaN > x is False
            best = True
            header["best_score"], header["best_row"] = float(score), row
    out[IS_BEST] = 1.0 if best else 0.0
    wm = NAN
    if conv_col >= 0 and row >= window - 1:
        s = 0.0
        for r in range(row - window + 1, row):  # oldest first
            s += table[r, conv_col]
        s += out[conv_col]
        wm = s / window
        if header["converged_row"] < 0 and wm > threshold:
            header["converged_row"] = row
    out[IDX["window_mean"]] = wm
    header["rows_written"] = row + 1
    table[row] = out
    return best


def series_rules(scores, episodes, min_episodes, conv_values, window, threshold):
    """Keep-best rows and the convergence row of whole series (one entry per row): the rows at
    which is_best is set, and converged_row (-1: none)."""
    table, header = np.zeros((len(scores), COLS)), new_header()
    best_rows = []
    for r, (s, e, c) in enumerate(zip(scores, episodes, conv_values)):
        v = {"episodes": float(e), "mean_return": s, "value_mean": c}
        if finish_row(table, header, r, v, IDX["mean_return"], min_episodes, IDX["value_mean"], window, threshold):
            best_rows.append(r)
    return best_rows, header, table
