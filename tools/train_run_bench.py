"""What a learning curve costs per iteration (config_easy, 4096 envs x 200 steps, the benchmark's size).

Three arms on one trainer, alternated over repeats, each timed with device events after a warm-up:
  a  a plain iteration() loop                                  (no curve)
  b  fit(poll_every=0)                                         (the curve kept on the device)
  c  the iteration() loop reading episode_stats() and loss_stats() every iteration
                                                               (the only way to a curve before fit)
Prints one JSON line: ms per iteration per arm (median, min, max over repeats).

--sharded measures the rank-merged log instead: a world-1 RCCL process group is created before any
GPU work (as bench.py --dist does), the trainer is collective, and two arms alternate:
  a  the plain iteration() loop on the collective trainer
  d  fit(merge_ranks=True)          (rank record, one all-gather over RCCL, the row from the records)

    python tools/train_run_bench.py [--iters 30] [--repeats 5] [--out FILE]
    python tools/train_run_bench.py --sharded [--repeats 7] [--out FILE]
    python tools/train_run_bench.py [--sharded] --profile   # a short fit for rocprofv3 --kernel-trace --stats
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
    p.add_argument("--sharded", action="store_true", help="a collective trainer on a world-1 RCCL group")
    a = p.parse_args()
    import torch
    from dexterous_rl_manipulation_amd import workloads
    dev = torch.device("cuda", 0)
    group = None
    if a.sharded:  # before any GPU work
        import datetime
        import socket
        import torch.distributed as dist
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(s.getsockname()[1]))
        s.close()
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", device_id=dev, rank=0, world_size=1, timeout=datetime.timedelta(seconds=120))
        group = dist.group.WORLD
    env, tr = workloads.build_pg_workload("easy", dev, envs=a.envs, horizon=a.horizon, process_group=group)
    try:
        measure(a, tr, dev)
    finally:
        if group is not None:
            torch.cuda.synchronize()
            dist.destroy_process_group()


def measure(a, tr, dev):
    import torch
    merge = dict(merge_ranks=True) if a.sharded else {}
    if a.profile:
        tr.fit(a.iters, **merge)
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

    def fit_merged():
        tr.fit(a.iters, poll_every=0, merge_ranks=True)

    arms = {"a_iteration": plain, "b_fit": fit, "c_iteration_host_stats": host_curve}
    if a.sharded:
        arms = {"a_iteration": plain, "d_fit_merge_ranks": fit_merged}
    tr.fit(a.warmup, **merge)
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
           "device": torch.cuda.get_device_name(dev), "sharded": bool(a.sharded)}
    for name, v in ms.items():
        res[name] = {"ms_per_iteration_median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
    other = "d_fit_merge_ranks" if a.sharded else "b_fit"
    res[other[:1] + "_minus_a_ms"] = res[other]["ms_per_iteration_median"] - res["a_iteration"]["ms_per_iteration_median"]
    res["a_spread_ms"] = res["a_iteration"]["max"] - res["a_iteration"]["min"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
