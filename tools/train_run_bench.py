"""What a learning curve costs per iteration (config_easy, 4096 envs x 200 steps, the benchmark's size).

Three arms on one trainer, alternated over repeats, each timed with device events after a warm-up:
  a  a plain iteration() loop                                  (no curve)
  b  fit(poll_every=0)                                         (the curve kept on the device)
  c  the iteration() loop reading episode_stats() and loss_stats() every iteration
                                                               (the only way to a curve before fit)
Prints one JSON line: ms per iteration per arm (median, min, max over repeats).

    python tools/train_run_bench.py [--iters 30] [--repeats 5] [--out FILE]
    python tools/train_run_bench.py --profile   # a short fit for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--horizon", type=int, default=200)
    p.add_argument("--out", default=None)
    p.add_argument("--profile", action="store_true")
    a = p.parse_args()
    import torch
    from dexterous_rl_manipulation_amd import workloads
    dev = torch.device("cuda", 0)
    env, tr = workloads.build_pg_workload("easy", dev, envs=a.envs, horizon=a.horizon)
    if a.profile:
        tr.fit(a.iters)
        torch.cuda.synchronize()
        return

    def plain():
        for _ in range(a.iters):
            tr.iteration()

    def fit():
        tr.fit(a.iters, poll_every=0)

    def host_curve():
        for _ in range(a.iters):
            tr.iteration()
            tr.episode_stats()
            tr.loss_stats()

    arms = {"a_iteration": plain, "b_fit": fit, "c_iteration_host_stats": host_curve}
    tr.fit(a.warmup)
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
    res = {"envs": a.envs, "horizon": a.horizon, "iters": a.iters, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(dev)}
    for name, v in ms.items():
        res[name] = {"ms_per_iteration_median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
    res["b_minus_a_ms"] = res["b_fit"]["ms_per_iteration_median"] - res["a_iteration"]["ms_per_iteration_median"]
    res["a_spread_ms"] = res["a_iteration"]["max"] - res["a_iteration"]["min"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
