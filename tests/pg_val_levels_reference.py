"""NumPy restatement of the noise-level validation row (include/dxrl.h, dxrl_pg_val_levels_row),
built on pg_val_reference.py: row_values on each level's slice of the level-major records, the
degradation columns with robustness_analysis.py's f64 operations in its order, the robust row
(sums in level order, then one division; strict comparisons seeded by level 0, so the first
extremum wins), and finish_row on the selected score."""
import numpy as np

import pg_val_reference as V

LEVEL_COLUMNS = ("obs_noise_std", "dyn_noise_std", "episodes", "successes", "success_rate", "mean_return",
                 "return_std", "mean_length", "mean_contacts", "min_object_success_rate", "degradation",
                 "degradation_percentage")
LEVEL_COLS = 12
LIDX = {name: k for k, name in enumerate(LEVEL_COLUMNS)}
STAT_COLUMNS = LEVEL_COLUMNS[2:10]  # the eight columns a level shares with the main row
ROBUST_COLUMNS = ("levels", "worst_level", "worst_success_rate", "mean_success_rate", "mean_noisy_success_rate",
                  "max_degradation", "max_degradation_percentage", "worst_mean_return")
ROBUST_COLS = 8
RIDX = {name: k for k, name in enumerate(ROBUST_COLUMNS)}
ROBUST_SCORES = ("worst_success_rate", "mean_success_rate", "mean_noisy_success_rate", "worst_mean_return")
MAX_LEVELS = 16
NAN = float("nan")


def level_slices(L, G, K):
    return [slice(l * G * K, (l + 1) * G * K) for l in range(L)]


def level_values(noise, G, K, ep_return, ep_length, ep_success, ep_contacts):
    """One dict per level: the level's noise, row_values' statistics on its slice, and the
    degradation columns against level 0."""
    rows = []
    for l, s in enumerate(level_slices(len(noise), G, K)):
        v = V.row_values(G, K, 0, 0, 0, np.asarray(ep_return)[s], np.asarray(ep_length)[s], np.asarray(ep_success)[s],
                         np.asarray(ep_contacts)[s])
        r = {"obs_noise_std": float(noise[l][0]), "dyn_noise_std": float(noise[l][1])}
        r.update({name: v[name] for name in STAT_COLUMNS})
        rows.append(r)
    return add_degradation(rows)


def add_degradation(rows):
    base = rows[0]["success_rate"]
    for r in rows:
        r["degradation"] = base - r["success_rate"]
        r["degradation_percentage"] = (r["degradation"] / base * 100) if base > 0 else 0.0
    return rows


def robust_values(rows):
    """The robust row of a list of level dicts (success_rate, mean_return and the degradation
    columns are read)."""
    L = len(rows)
    worst_level, worst_rate = 0, rows[0]["success_rate"]
    max_deg, max_pct, worst_return = 0.0, 0.0, rows[0]["mean_return"]
    sum_all = sum_noisy = 0.0
    for l, r in enumerate(rows):
        sum_all += r["success_rate"]
        if l > 0:
            sum_noisy += r["success_rate"]
            if r["success_rate"] < worst_rate:
                worst_level, worst_rate = l, r["success_rate"]
            if r["degradation"] > max_deg:
                max_deg = r["degradation"]
            if r["degradation_percentage"] > max_pct:
                max_pct = r["degradation_percentage"]
            if r["mean_return"] < worst_return:
                worst_return = r["mean_return"]
    return {"levels": float(L), "worst_level": float(worst_level), "worst_success_rate": worst_rate,
            "mean_success_rate": sum_all / L, "mean_noisy_success_rate": sum_noisy / (L - 1) if L > 1 else NAN,
            "max_degradation": max_deg, "max_degradation_percentage": max_pct, "worst_mean_return": worst_return}


def level_array(rows):
    return np.array([[r[name] for name in LEVEL_COLUMNS] for r in rows], dtype=np.float64)


def robust_array(rob):
    return np.array([rob[name] for name in ROBUST_COLUMNS], dtype=np.float64)


def levels_row(noise, G, K, iteration, env_steps, train_row, ep_return, ep_length, ep_success, ep_contacts, status=0,
               solve_threshold=1.0):
    """(main row values of level 0, level dicts, robust dict)."""
    s0 = level_slices(1, G, K)[0]
    main = V.row_values(G, K, iteration, env_steps, train_row, np.asarray(ep_return)[s0], np.asarray(ep_length)[s0],
                        np.asarray(ep_success)[s0], np.asarray(ep_contacts)[s0], status, solve_threshold)
    rows = level_values(noise, G, K, ep_return, ep_length, ep_success, ep_contacts)
    return main, rows, robust_values(rows)


def selected_score(main, rob, score_table, score_col):
    if score_col < 0:
        return NAN
    return robust_array(rob)[score_col] if score_table else main[V.COLUMNS[score_col]]


def finish_levels_row(table, header, row, main, rob, score_table=0, score_col=-1, min_delta=0.0, patience=0):
    """V.finish_row with the selected score: writes table[row] (the main row) and applies the header
    rules; returns is_best."""
    if score_col < 0 or not score_table:
        return V.finish_row(table, header, row, main, score_col, min_delta, patience)
    # the rules read the score from the row they are given: lend the robust score a main-row slot
    carrier = V.IDX["mean_return"]
    lent = dict(main, mean_return=robust_array(rob)[score_col])
    best = V.finish_row(table, header, row, lent, carrier, min_delta, patience)
    table[row, carrier] = main.get("mean_return", 0.0)
    return best


def robust_series(scores, min_delta=0.0, patience=0, statuses=None):
    """Keep-best rows and header of a series of robust scores (V.series_rules: the rules do not
    depend on which table the score came from)."""
    best, header, table = V.series_rules(scores, min_delta, patience, statuses)
    return best, header, table[:, [V.IS_BEST, V.SINCE_BEST]]


def nan_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def level_results(noise, rows):
    """RobustnessTester-order result dictionaries of one table row's levels."""
    return [{"noise_levels": {"observation_noise_std": float(o), "dynamics_noise_std": float(d)},
             "metrics": {name: r[name] for name in LEVEL_COLUMNS[2:]}} for (o, d), r in zip(noise, rows)]
