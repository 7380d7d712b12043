"""NumPy restatement of the held-out validation row and its header rules (include/dxrl.h,
dxrl_pg_val_row).  Sums are plain f64 sums, the standard deviation two-pass f64 -- the
definitions, not the device's summation order."""
import math

import numpy as np

COLUMNS = ("iteration", "env_steps", "train_row", "episodes", "successes", "success_rate", "mean_return",
           "return_std", "mean_length", "mean_success_length", "mean_contacts", "min_object_success_rate",
           "objects_solved", "eval_status", "is_best", "since_best")
COLS = 16
IDX = {name: k for k, name in enumerate(COLUMNS)}
IS_BEST = IDX["is_best"]
SINCE_BEST = IDX["since_best"]
NAN = float("nan")


def new_header():
    return {"rows_written": 0, "best_row": -1, "stopped_row": -1, "since_best": 0, "best_score": -math.inf}


def two_pass_std(x):
    x = np.asarray(x, dtype=np.float64)
    return math.sqrt(float(np.mean((x - x.mean()) ** 2)))


def object_successes(G, K, ep_success):
    """i64 [G]: successes of object o = non-zero bytes of records [o K, (o + 1) K)."""
    s = np.asarray(ep_success)[:G * K].reshape(G, K)
    return np.count_nonzero(s, axis=1).astype(np.int64)


def row_values(G, K, iteration, env_steps, train_row, ep_return, ep_length, ep_success, ep_contacts, status=0,
               solve_threshold=1.0):
    """Columns before is_best, as a dict.  Only the first G * K records are read."""
    E = G * K
    ret = np.asarray(ep_return, dtype=np.float64)[:E]
    length = np.asarray(ep_length, dtype=np.int64)[:E]
    suc = np.asarray(ep_success)[:E] != 0
    con = np.asarray(ep_contacts, dtype=np.int64)[:E]
    per_object = object_successes(G, K, ep_success)
    n_suc = int(suc.sum())
    out = {"iteration": float(iteration), "env_steps": float(env_steps), "train_row": float(train_row),
           "episodes": float(E), "successes": float(n_suc), "success_rate": n_suc / E,
           "mean_return": float(ret.sum()) / E, "return_std": two_pass_std(ret),
           "mean_length": int(length.sum()) / E,
           "mean_success_length": int(length[suc].sum()) / n_suc if n_suc else NAN,
           "mean_contacts": int(con.sum()) / E,
           "min_object_success_rate": int(per_object.min()) / K,
           "objects_solved": float(sum(1 for c in per_object.tolist() if c / K >= solve_threshold)),
           "eval_status": float(status)}
    return out


def finish_row(table, header, row, values, score_col=-1, min_delta=0.0, patience=0):
    """Write `values` (row_values' dict) as table[row] and apply keep-best and patience to `header`
    in place.  Returns the is_best flag."""
    out = np.zeros(COLS)
    for name, v in values.items():
        out[IDX[name]] = v
    best = False
    if score_col >= 0:
        score = out[score_col]
        if values.get("eval_status", 0.0) == 0 and score > header["best_score"] + min_delta:  # NaN > x is False
            best = True
            header["best_score"], header["best_row"] = float(score), row
    since = 0 if best else header["since_best"] + 1
    out[IS_BEST], out[SINCE_BEST] = (1.0 if best else 0.0), float(since)
    header["since_best"] = since
    if patience > 0 and header["stopped_row"] < 0 and since >= patience:
        header["stopped_row"] = row
    header["rows_written"] = row + 1
    table[row] = out
    return best


def series_rules(scores, min_delta=0.0, patience=0, statuses=None, score_name="mean_return"):
    """Keep-best rows, the header and the table of a whole series of scores (one per row)."""
    table, header = np.zeros((len(scores), COLS)), new_header()
    best_rows = []
    for r, s in enumerate(scores):
        v = {score_name: s, "eval_status": 0.0 if statuses is None else float(statuses[r])}
        if finish_row(table, header, r, v, IDX[score_name], min_delta, patience):
            best_rows.append(r)
    return best_rows, header, table
