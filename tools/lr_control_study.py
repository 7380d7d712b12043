"""What step-size control does to a run: python tools/lr_control_study.py [iterations target_kl]

Hard curriculum, 4096 envs x 200 steps, 4 epochs x 4 minibatches, validation every 20 iterations,
seeds 42 / 123 / 456, through run_training_study: arm `plain` (lr 3e-4) against arm `kl` (the same
lr with target_kl and kl_adaptive).  Reports held-out final-window success per run and arm, the
kl_epoch and lr curves and the stops per run.  Writes bench_out/lr_control/study.json
(profiles/lr_control/ keeps a copy)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexterous_rl_manipulation_amd import training_study as T  # noqa: E402

ITER = int(sys.argv[1]) if len(sys.argv) > 1 else 200
TARGET = float(sys.argv[2]) if len(sys.argv) > 2 else 0.01
SEEDS = (42, 123, 456)
WIN = 3  # validation rows per final window


def main():
    arms = [T.Arm("plain", False, "dense", "hard"),
            T.Arm("kl", False, "dense", "hard", trainer_kw=dict(target_kl=TARGET, kl_adaptive=True))]
    spec = (T.Spec("success_rate", window=WIN, final_window=WIN),)
    t0 = time.perf_counter()
    res = T.run_training_study(arms, SEEDS, ITER, num_envs=4096, horizon=200, max_steps=200, validate_every=20,
                               train_specs=(T.Spec("success_rate"),), val_specs=spec, return_logs=True,
                               contrasts={"kl_minus_plain": {"kl": 1.0, "plain": -1.0}}, lr=3e-4, epochs=4,
                               minibatches=4)
    wall = time.perf_counter() - t0
    out = {"iterations": ITER, "target_kl": TARGET, "seeds": list(SEEDS), "wall_s": wall, "runs": []}
    r = 0
    for arm in arms:
        for seed in SEEDS:
            log = res.logs[r]
            r += 1
            val = log.validation["success_rate"]
            run = {"arm": arm.name, "seed": seed, "heldout_success": val.tolist(),
                   "heldout_final_window": float(np.mean(val[-WIN:])),
                   "train_success_last10": float(np.nanmean(log["success_rate"][-10:])),
                   "approx_kl_last_pass_mean": float(np.mean(log["approx_kl"]))}
            if log.optimizer is not None:
                o = log.optimizer
                run.update(stops=int((o.column("stop_pass") >= 0).sum()), skipped=int(o.column("skipped").sum()),
                           kl_epoch=o.column("kl_epoch")[::10].tolist(), lr=o.column("lr")[::10].tolist(),
                           lr_final=float(o.column("lr")[-1]), lr_min_seen=float(o.column("lr").min()),
                           lr_max_seen=float(o.column("lr").max()))
            out["runs"].append(run)
    for arm in arms:
        v = [x["heldout_final_window"] for x in out["runs"] if x["arm"] == arm.name]
        out[f"{arm.name}_heldout_final_window_mean"] = float(np.mean(v))
        out[f"{arm.name}_heldout_final_window_std"] = float(np.std(v, ddof=1))
    d = os.path.join(ROOT, "bench_out", "lr_control")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "study.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    for x in out["runs"]:
        print(json.dumps({k: x[k] for k in x if k not in ("heldout_success", "kl_epoch", "lr")}))


if __name__ == "__main__":
    main()
