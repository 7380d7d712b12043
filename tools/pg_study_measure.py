"""Measurements of the PG ablation study at config_easy size: 4096 envs x 200 steps, 4 arms x 3 seeds
x 200 iterations, validation every 20 (python tools/pg_study_measure.py [repeats iterations]):
the runner's wall time per iteration against fit() alone in the same process (alternated), the
device summary against the NumPy one, and the 2 x 2 table itself.  Writes
bench_out/pg_study/*.json / *.txt (profiles/pg_study/ keeps a copy).  tools/pg_study_trace.py is the
program for the rocprofv3 --kernel-trace run of the three summary launches."""
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexterous_rl_manipulation_amd import ablation, training_study as T  # noqa: E402

OUT = os.path.join(ROOT, "bench_out", "pg_study")
os.makedirs(OUT, exist_ok=True)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ITER = int(sys.argv[2]) if len(sys.argv) > 2 else 200
SEEDS = (42, 123, 456)
JOB = dict(num_envs=4096, horizon=200, max_steps=200, validate_every=20)
WIN = 3  # validation rows (every 20 iterations) per window
SPECS = ablation.pg_study_specs(WIN, 0.5, WIN)
T_START = time.perf_counter()


def sync():
    torch.cuda.synchronize()


def study():
    sync()
    t0 = time.perf_counter()
    stats, result = ablation.run_pg_component_study(ITER, SEEDS, return_study=True, convergence_window=WIN,
                                                    final_window=WIN, **JOB)
    result.training.run_table, result.validation.run_table  # the lazy copy
    sync()
    return time.perf_counter() - t0, stats, result


def plain():
    """fit() alone, per arm (seed 42): the trainer is built before the clock starts."""
    per_arm = []
    for arm in ablation.pg_component_arms():
        env, tr, fit_kw = T.make_job(arm, 42, train_spec=SPECS[0], **JOB)
        sync()
        t0 = time.perf_counter()
        log = tr.fit(ITER, **fit_kw)
        log.table
        sync()
        per_arm.append((time.perf_counter() - t0) / ITER)
        T.release_job(env, tr, fit_kw)
        del env, tr, fit_kw, log
    return per_arm


# warm-up: code objects, allocator
ablation.run_pg_component_study(3, (42,), num_envs=4096, horizon=200, max_steps=200, validate_every=2)
sync()
rows = []
stats = result = None
for rep in range(REPS):
    order = ("study", "plain") if rep % 2 == 0 else ("plain", "study")
    rec = {"rep": rep, "order": order}
    for what in order:
        if what == "study":
            dt, stats, result = study()
            rec["study_s"] = dt
            rec["study_ms_per_iteration"] = 1e3 * dt / (4 * len(SEEDS) * ITER)
        else:
            per_arm = plain()
            rec["plain_ms_per_iteration_by_arm"] = [1e3 * x for x in per_arm]
            rec["plain_ms_per_iteration"] = 1e3 * float(np.mean(per_arm))
    rec["overhead_percent"] = 100.0 * (rec["study_ms_per_iteration"] / rec["plain_ms_per_iteration"] - 1.0)
    rows.append(rec)
    print(json.dumps(rec), flush=True)
    if time.perf_counter() - T_START > 560:
        print("time guard: stopping after", rep + 1, "repeats", flush=True)
        break
rng = lambda k: [min(r[k] for r in rows), max(r[k] for r in rows)]  # noqa: E731
overhead = {"iterations": ITER, "seeds": list(SEEDS), "job": JOB, "repeats": rows,
            "study_ms_per_iteration_range": rng("study_ms_per_iteration"),
            "plain_ms_per_iteration_range": rng("plain_ms_per_iteration"),
            "overhead_percent_range": rng("overhead_percent")}
json.dump(overhead, open(os.path.join(OUT, "runner_overhead.json"), "w"), indent=2)

# the summary: device against host, on the last study's slabs
arms = result.arms
off, flat = T.csr_groups([[a * len(SEEDS) + k for k in range(len(SEEDS))] for a in range(len(arms))])
weights = T.contrast_matrix(arms, ablation.PG_COMPONENT_CONTRASTS)
summary = {}
for mode in ("device", "host"):
    times, nbytes = [], 0
    for rep in range(21):
        sync()
        t0 = time.perf_counter()
        nbytes = 0
        for name in T.SLABS:
            nat = T.native_specs(SPECS, name)
            if mode == "device":
                pending, nb = T.summarize_device(result.slabs[name], result.run_rows[name], nat, off, flat, weights)
                s = T.SlabSummary(name, SPECS, result.run_names, arms, list(ablation.PG_COMPONENT_CONTRASTS),
                                  _pending=pending)
                s.run_table
            else:
                host = result.slabs[name].cpu().numpy()
                nb = host.nbytes
                T.summarize_host(host, result.run_rows[name], nat, off, flat, weights)
            nbytes += nb
        sync()
        times.append(1e3 * (time.perf_counter() - t0))
    times = times[1:]
    summary[mode] = {"ms_range": [min(times), max(times)], "ms_median": float(np.median(times)),
                     "bytes_to_host": nbytes, "repeats": len(times)}
    print(mode, summary[mode], flush=True)
json.dump(summary, open(os.path.join(OUT, "summary_device_vs_host.json"), "w"), indent=2)

# the 2 x 2 itself (hard config, held-out validation)
buf = io.StringIO()
with redirect_stdout(buf):
    ablation.print_ablation_report({}, stats)
    from dexterous_rl_manipulation_amd import pg_ablation
    print("\n".join(pg_ablation.effect_lines(stats)))
open(os.path.join(OUT, "ablation_hard_200.txt"), "w").write(buf.getvalue())
json.dump(pg_ablation.results_json(stats, result), open(os.path.join(OUT, "ablation_hard_200.json"), "w"), indent=1,
          allow_nan=False)
print(buf.getvalue())
