"""Cost of value normalisation at config_easy size (4096 envs x 200 steps):
python tools/value_norm_bench.py [repeats iterations] [--trace ARM]

Two trainers in one process, alternated: `plain` (dxrl_pg_gae) and `value_norm`
(TrainerConfig.value_norm: dxrl_pg_gae_vnorm, which also stores ret_norm and values_raw and reduces
a second moments triple).  Each repeat times the advantages phase alone (HIP events around 40
back-to-back calls, as tools/phase_time.py does) and `iterations` whole iterations of each arm
between two synchronisations.  Writes bench_out/value_norm/cost.json (profiles/value_norm/ keeps a
copy).

--trace ARM: warm up, then run 30 iterations of one arm and exit -- the program of a
rocprofv3 --kernel-trace --stats run."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexterous_rl_manipulation_amd import workloads  # noqa: E402

TRACE = sys.argv[sys.argv.index("--trace") + 1] if "--trace" in sys.argv else None
ARGS = [a for a in sys.argv[1:] if not a.startswith("--") and a != TRACE]
REPS = int(ARGS[0]) if ARGS else 7
ITER = int(ARGS[1]) if len(ARGS) > 1 else 30
CALLS = 40
ARMS = {"plain": {}, "value_norm": dict(value_norm=True)}


def build(name):
    env, tr = workloads.build_pg_workload("easy", None, **ARMS[name])
    for _ in range(3):
        tr.iteration()
    torch.cuda.synchronize()
    return env, tr


def timed(tr):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITER):
        tr.iteration()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITER * 1e3


def phase_us(tr):
    """(Repeated advantages() calls fold the same returns again: the timing arm's state is not a
    training run's, and the whole-iteration timings run before it within a repeat.)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tr.advantages()
    a.record()
    for _ in range(CALLS):
        tr.advantages()
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
    us = {name: [] for name in ARMS}
    for _ in range(REPS):
        for name, (_, tr) in trainers.items():
            ms[name].append(timed(tr))
        for name, (_, tr) in trainers.items():
            us[name].append(phase_us(tr))
    out = {"size": "4096 envs x 200 steps, 1 x 1", "repeats": REPS, "iterations": ITER, "phase_calls": CALLS,
           "advantages_us": us, "ms_per_iteration": ms,
           "median_advantages_us": {k: statistics.median(v) for k, v in us.items()},
           "median_ms": {k: statistics.median(v) for k, v in ms.items()},
           "spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
           "advantages_value_norm_minus_plain_us": [a - b for a, b in zip(us["value_norm"], us["plain"])],
           "iteration_value_norm_minus_plain_us": [1e3 * (a - b) for a, b in zip(ms["value_norm"], ms["plain"])],
           "value_norm_state": trainers["value_norm"][1].value_norm_state()}
    d = os.path.join(ROOT, "bench_out", "value_norm")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "cost.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("advantages_us", "ms_per_iteration")}))


if __name__ == "__main__":
    main()
