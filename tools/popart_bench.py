"""Cost of PopArt at config_easy size (4096 envs x 200 steps):
python tools/popart_bench.py [repeats iterations] [--trace ARM]

Two trainers in one process, alternated: `value_norm` and `popart` (TrainerConfig.popart: one
dxrl_pg_popart_rescale launch behind the iteration's last optimiser step).  Each repeat times
`iterations` whole iterations of each arm between two HIP events, and the rescale alone (HIP events
around 40 back-to-back calls; after the first they take the no-op path, which still reads both
blocks and is the launch's floor).  Writes bench_out/popart/cost.json (profiles/popart/ keeps a
copy).

--trace ARM: warm up, then run 30 iterations of one arm and exit -- the program of a
rocprofv3 --kernel-trace --stats run."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexterous_rl_manipulation_amd import workloads  # noqa: E402

TRACE = sys.argv[sys.argv.index("--trace") + 1] if "--trace" in sys.argv else None
ARGS = [a for a in sys.argv[1:] if not a.startswith("--") and a != TRACE]
REPS = int(ARGS[0]) if ARGS else 7
ITER = int(ARGS[1]) if len(ARGS) > 1 else 30
CALLS = 40
ARMS = {"value_norm": dict(value_norm=True), "popart": dict(value_norm=True, popart=True)}


def build(name):
    env, tr = workloads.build_pg_workload("easy", None, **ARMS[name])
    for _ in range(3):
        tr.iteration()
    torch.cuda.synchronize()
    return env, tr


def timed(tr):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(ITER):
        tr.iteration()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITER


def rescale_us(tr):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tr.popart_rescale()
    a.record()
    for _ in range(CALLS):
        tr.popart_rescale()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3


def main():
    if TRACE:
        _, tr = build(TRACE)
        timed(tr)
        return
    trainers = {name: build(name) for name in ARMS}
    ms = {name: [] for name in ARMS}
    us = []
    for _ in range(REPS):
        for name, (_, tr) in trainers.items():
            ms[name].append(timed(tr))
        us.append(rescale_us(trainers["popart"][1]))
    out = {"size": "4096 envs x 200 steps, 1 x 1", "repeats": REPS, "iterations": ITER, "rescale_calls": CALLS,
           "ms_per_iteration": ms, "rescale_us": us,
           "median_ms": {k: statistics.median(v) for k, v in ms.items()},
           "spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
           "median_rescale_us": statistics.median(us),
           "iteration_popart_minus_value_norm_us": [1e3 * (a - b) for a, b in zip(ms["popart"], ms["value_norm"])],
           "popart_state": trainers["popart"][1].popart_state()}
    d = os.path.join(ROOT, "bench_out", "popart")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "cost.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "ms_per_iteration"}))


if __name__ == "__main__":
    main()
