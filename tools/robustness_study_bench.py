"""A robustness sweep summarised on the device and analysed on the host, against the device study.

    python tools/robustness_study_bench.py [--episodes 3150] [--max-episode-steps 200] [--rounds 7]
                                           [--config hard] [--out FILE]

The sweep is observation levels [0, 0.05, 0.1] x dynamics levels [0, 0.05, 0.1] = 13 levels of
--episodes episodes each (default 13 x 3,150 = 40,950, the nearest to the other studies' 40,960)
of the deterministic MLP actor, device Philox resets and noise, run in one process:

  sweep   run_robustness_sweep(parallel=True, device_summary=True), then
          analyze_robustness_results: the episode launch writes contact_hist, dxrl_eval_summarize
          reads it back; the degradation columns are formed on the host;
  study   run_robustness_study: the episode kernel accumulates the history moments, no history is
          allocated; dxrl_robustness_summarize forms the group tables and the degradation columns.

The two forms alternate within a round (one warm-up round first, then --rounds timed rounds); per
form: wall clock around the whole call, HIP-event time of the episode kernel and of the summary
launches, the bytes copied to the host and the device bytes allocated for the episode records and
the summary's buffers; median, min and max over the rounds.  Writes one JSON file.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from seed_variance_bench import actor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=3150)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--config", default="hard")
    ap.add_argument("--out", default=os.path.join("profiles", "robustness_study", "bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import evaluation as ev, evaluator as evr, robustness_analysis as ra

    T, K = a.max_episode_steps, a.episodes
    obs = dyn = [0.0, 0.05, 0.1]
    cfg = getattr(pkg.CurriculumConfig, a.config)()
    pol = actor()
    rt = ev.RobustnessTester(pol, cfg, max_episode_steps=T)

    # the launch of each call, to read its event times and its buffers
    last = {}
    real_launch = evr.EpisodeProgram.launch

    def launch(self, *args, **kw):
        pending = real_launch(self, *args, **kw)
        take = pending.result

        def result(timing=None):
            tm = {} if timing is None else timing
            out = take(tm)
            last.update(timing=dict(tm), host_bytes=out.host_bytes)
            return out

        pending.result = result
        tensors = {x.data_ptr(): x for x in list(pending.outs) + pending.summary.tensors if x is not None}
        last["device_bytes"] = sum(x.numel() * x.element_size() for x in tensors.values())
        return pending

    evr.EpisodeProgram.launch = launch

    def sweep():
        res = rt.run_robustness_sweep(obs, dyn, K, 0, parallel=True, device_seed=0, device_summary=True)
        return ra.analyze_robustness_results(res)

    def study():
        return ra.run_robustness_study(pol, cfg, obs, dyn, K, 0, parallel=True, device_seed=0,
                                       max_episode_steps=T)["analysis"]

    forms = [("sweep", sweep), ("study", study)]
    runs = {name: [] for name, _ in forms}
    analyses = {}
    for rnd in range(-1, a.rounds):  # round -1: warm-up of both forms
        for name, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            analyses[name] = fn()
            torch.cuda.synchronize()
            r = {"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": last["timing"]["kernel_ms"],
                 "summary_ms": last["timing"]["summary_ms"], "host_bytes": last["host_bytes"],
                 "device_bytes": last["device_bytes"]}
            if rnd >= 0:
                runs[name].append(r)
                print(json.dumps({"round": rnd, "form": name, "wall_ms": round(r["wall_ms"], 3),
                                  "kernel_ms": round(r["kernel_ms"], 4), "summary_ms": round(r["summary_ms"], 4)}),
                      flush=True)

    def spread(xs):
        return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}

    levels = len(rt.sweep_levels(obs, dyn)[0])
    out = {"study": {"levels": levels, "episodes_per_level": K, "max_episode_steps": T,
                     "total_episodes": levels * K, "policy": "deterministic MLP actor", "config": a.config,
                     "device": torch.cuda.get_device_name(0)},
           "analyses_equal": analyses["sweep"] == analyses["study"], "forms": {}}
    for name, rs in runs.items():
        out["forms"][name] = {
            "rounds": len(rs), "wall_ms": spread([r["wall_ms"] for r in rs]),
            "episode_kernel_ms": spread([r["kernel_ms"] for r in rs]),
            "summary_ms": spread([r["summary_ms"] for r in rs]),
            "host_ms": spread([r["wall_ms"] - r["kernel_ms"] - r["summary_ms"] for r in rs]),
            "host_bytes": rs[-1]["host_bytes"], "device_record_bytes": rs[-1]["device_bytes"]}
    sk, dk = ([r["kernel_ms"] for r in runs[n]] for n in ("sweep", "study"))
    out["episode_kernel_ab"] = {
        "history_ms": spread(sk), "moments_ms": spread(dk),
        "moments_minus_history_ms": round(statistics.median(dk) - statistics.median(sk), 4),
        "round_spread_ms": round(max(max(sk) - min(sk), max(dk) - min(dk)), 4)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
