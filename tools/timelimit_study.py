"""What the time-limit bootstrap does to a run: python tools/timelimit_study.py [iterations]

Hard curriculum, dense reward, 4096 envs x 200 steps, held-out validation every 20 iterations,
seeds 42 / 123 / 456: `plain` against `bootstrap` (TrainerConfig.timeout_bootstrap), each job
training_study.make_job's env, trainer and fit arguments.  Reports per run the explained variance
and value loss over the run (each arm against its own value targets), the share of an iteration's
samples that belong to episodes cut by the time limit (from the log: episodes x (1 - success_rate)
x max_steps / samples -- under success_rule "terminated" every unsuccessful end is a time limit --
and, on the bootstrap arm, from timeout_stats() of the last iteration) and the held-out
final-window success.  Writes bench_out/timelimit/study.json (profiles/timelimit/ keeps a copy)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexterous_rl_manipulation_amd import training_study as T  # noqa: E402

ITER = int(sys.argv[1]) if len(sys.argv) > 1 else 200
SEEDS = (42, 123, 456)
ENVS, HORIZON, MAX_STEPS = 4096, 200, 200
WIN = 3  # validation rows per final window
ARMS = {"plain": {}, "bootstrap": dict(timeout_bootstrap=True)}


def thirds(col):
    """Means over the first, middle and last third of the run (NaN rows left out)."""
    return [float(np.nanmean(p)) for p in np.array_split(np.asarray(col, dtype=np.float64), 3)]


def main():
    out = {"iterations": ITER, "seeds": list(SEEDS), "size": f"{ENVS} envs x {HORIZON} steps, max_steps {MAX_STEPS}",
           "runs": []}
    t0 = time.perf_counter()
    for name, kw in ARMS.items():
        for seed in SEEDS:
            job = T.make_job(T.Arm(name, False, "dense", "hard"), seed, num_envs=ENVS, horizon=HORIZON,
                             max_steps=MAX_STEPS, validate_every=20, **kw)
            env, tr, fit_kw = job
            log = tr.fit(ITER, **fit_kw)
            val = log.validation["success_rate"]
            cut = log["episodes"] * (1.0 - log["success_rate"]) * MAX_STEPS / (ENVS * HORIZON)
            run = {"arm": name, "seed": seed, "heldout_success": val.tolist(),
                   "heldout_final_window": float(np.mean(val[-WIN:])),
                   "train_success_last10": float(np.nanmean(log["success_rate"][-10:])),
                   "explained_variance_thirds": thirds(log["explained_variance"]),
                   "explained_variance_last10": float(np.nanmean(log["explained_variance"][-10:])),
                   "value_mse_thirds": thirds(log["value_mse"]),
                   "value_mse_last10": float(np.nanmean(log["value_mse"][-10:])),
                   "target_var_last10": float(np.nanmean(log["target_var"][-10:])),
                   "target_mean_last10": float(np.nanmean(log["target_mean"][-10:])),
                   "grad_norm_last10": float(np.nanmean(log["grad_norm"][-10:])),
                   "time_limit_sample_share_thirds": thirds(cut),
                   "time_limit_sample_share_last10": float(np.nanmean(cut[-10:]))}
            if tr.cfg.timeout_bootstrap:
                st = tr.timeout_stats()
                run["timeout_stats_last_iteration"] = st
                run["time_limit_sample_share_last_iteration"] = st["timeouts"] * MAX_STEPS / (ENVS * HORIZON)
                run["log_ends_last_iteration"] = float(log["episodes"][-1])
            out["runs"].append(run)
            T.release_job(*job)
    out["wall_s"] = time.perf_counter() - t0
    for name in ARMS:
        for key in ("heldout_final_window", "explained_variance_last10", "value_mse_last10",
                    "time_limit_sample_share_last10"):
            v = [x[key] for x in out["runs"] if x["arm"] == name]
            out[f"{name}_{key}_mean"] = float(np.mean(v))
            out[f"{name}_{key}_std"] = float(np.std(v, ddof=1))
    d = os.path.join(ROOT, "bench_out", "timelimit")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "study.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    for x in out["runs"]:
        print(json.dumps({k: x[k] for k in x if k != "heldout_success"}))


if __name__ == "__main__":
    main()
