"""What value normalisation does to a run: python tools/value_norm_study.py [iterations]

Hard curriculum, dense reward, 4096 envs x 200 steps, held-out validation every 20 iterations,
seeds 42 / 123 / 456: TrainerConfig.value_norm off and on, each without and with
timeout_bootstrap (four arms), each job training_study.make_job's env, trainer and fit arguments.
Reports per run, over the last ten iterations, the explained variance, residual_var (the raw value
error: value_mse is in normalised units on the value_norm arms), grad_norm before clipping and the
share of iterations whose clip factor min(1, max_grad_norm / grad_norm) is below 1, and the held-out
final-window success.  Writes bench_out/value_norm/study.json (profiles/value_norm/ keeps a copy)."""
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
ARMS = {"plain": {}, "value_norm": dict(value_norm=True), "bootstrap": dict(timeout_bootstrap=True),
        "bootstrap_value_norm": dict(timeout_bootstrap=True, value_norm=True)}
KEYS = ("heldout_final_window", "train_success_last10", "explained_variance_last10", "residual_var_last10",
        "target_var_last10", "value_mse_last10", "grad_norm_last10", "clipped_share_last10", "clip_factor_last10")


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
            last = lambda col: float(np.nanmean(np.asarray(log[col], dtype=np.float64)[-10:]))  # noqa: E731
            gn = np.asarray(log["grad_norm"], dtype=np.float64)[-10:]
            run = {"arm": name, "seed": seed, "heldout_success": val.tolist(),
                   "heldout_final_window": float(np.mean(val[-WIN:])),
                   "train_success_last10": last("success_rate"),
                   "explained_variance_last10": last("explained_variance"),
                   "residual_var_last10": last("residual_var"), "target_var_last10": last("target_var"),
                   "target_mean_last10": last("target_mean"), "value_mse_last10": last("value_mse"),
                   "grad_norm_last10": float(gn.mean()),
                   "clipped_share_last10": float((gn > tr.cfg.max_grad_norm).mean()),
                   "clip_factor_last10": float(np.minimum(1.0, tr.cfg.max_grad_norm / gn).mean())}
            if tr.cfg.value_norm:
                run["value_norm_state"] = tr.value_norm_state()
            out["runs"].append(run)
            T.release_job(*job)
    out["wall_s"] = time.perf_counter() - t0
    for name in ARMS:
        for key in KEYS:
            v = [x[key] for x in out["runs"] if x["arm"] == name]
            out[f"{name}_{key}_mean"] = float(np.mean(v))
            out[f"{name}_{key}_std"] = float(np.std(v, ddof=1))
    d = os.path.join(ROOT, "bench_out", "value_norm")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "study.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    for x in out["runs"]:
        print(json.dumps({k: x[k] for k in x if k != "heldout_success"}))


if __name__ == "__main__":
    main()
