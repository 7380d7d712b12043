"""What PopArt and the forgetting factor do to a value-normalised run:
python tools/popart_study.py [iterations]

Hard curriculum, dense reward, 4096 envs x 200 steps, held-out validation every 20 iterations,
seeds 42 / 123 / 456.  Arms: value_norm alone, + popart, + forget (value_norm_forget = 0.05),
+ both, each without and with timeout_bootstrap (eight arms), each job training_study.make_job's
env, trainer and fit arguments.  Reports per run, over the first twenty and the last ten
iterations, the explained variance, residual_var (the raw value error) and value_mse (normalised
units); the mean per-iteration |shift| and |scale - 1| of the moving pair (from log.value_norm,
so on the popart arms only: the others keep no per-iteration record of the pair); and the held-out
final-window success.  Writes bench_out/popart/study.json (profiles/popart/ keeps a copy)."""
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
FORGET = 0.05
BASE = {"value_norm": {}, "popart": dict(popart=True), "forget": dict(value_norm_forget=FORGET),
        "popart_forget": dict(popart=True, value_norm_forget=FORGET)}
ARMS = {name: dict(value_norm=True, **kw) for name, kw in BASE.items()}
ARMS.update({"bootstrap_" + name: dict(value_norm=True, timeout_bootstrap=True, **kw) for name, kw in BASE.items()})
KEYS = ("heldout_final_window", "explained_variance_first20", "explained_variance_last10", "residual_var_first20",
        "residual_var_last10", "value_mse_first20", "value_mse_last10")
MOVES = ("abs_shift_first20", "abs_shift_last10", "abs_scale_minus_1_first20", "abs_scale_minus_1_last10")


def main():
    out = {"iterations": ITER, "seeds": list(SEEDS), "size": f"{ENVS} envs x {HORIZON} steps, max_steps {MAX_STEPS}",
           "forget": FORGET, "runs": []}
    t0 = time.perf_counter()
    for name, kw in ARMS.items():
        for seed in SEEDS:
            job = T.make_job(T.Arm(name, False, "dense", "hard"), seed, num_envs=ENVS, horizon=HORIZON,
                             max_steps=MAX_STEPS, validate_every=20, **kw)
            env, tr, fit_kw = job
            log = tr.fit(ITER, **fit_kw)
            val = log.validation["success_rate"]
            col = lambda c: np.asarray(log[c], dtype=np.float64)  # noqa: E731
            run = {"arm": name, "seed": seed, "heldout_success": val.tolist(),
                   "heldout_final_window": float(np.mean(val[-WIN:])), "value_norm_state": tr.value_norm_state()}
            for c in ("explained_variance", "residual_var", "value_mse"):
                run[c + "_first20"] = float(np.nanmean(col(c)[:20]))
                run[c + "_last10"] = float(np.nanmean(col(c)[-10:]))
            if tr.cfg.popart:
                vn = log.value_norm
                run.update(abs_shift_first20=float(np.abs(vn["shift"][:20]).mean()),
                           abs_shift_last10=float(np.abs(vn["shift"][-10:]).mean()),
                           abs_scale_minus_1_first20=float(np.abs(vn["scale"][:20] - 1.0).mean()),
                           abs_scale_minus_1_last10=float(np.abs(vn["scale"][-10:] - 1.0).mean()),
                           popart_state=tr.popart_state())
            out["runs"].append(run)
            T.release_job(*job)
    out["wall_s"] = time.perf_counter() - t0
    for name in ARMS:
        runs = [x for x in out["runs"] if x["arm"] == name]
        for key in KEYS + (MOVES if "popart" in name else ()):
            v = [x[key] for x in runs]
            out[f"{name}_{key}_mean"] = float(np.mean(v))
            out[f"{name}_{key}_std"] = float(np.std(v, ddof=1))
    d = os.path.join(ROOT, "bench_out", "popart")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "study.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    for x in out["runs"]:
        print(json.dumps({k: x[k] for k in x if k != "heldout_success"}))


if __name__ == "__main__":
    main()
