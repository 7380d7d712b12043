"""A failure-mode study on the host pipeline against the device study.

    python tools/failure_study_bench.py [--objects 64] [--episodes 640] [--max-episode-steps 200]
                                        [--classify-max-steps 400] [--rounds 7] [--out FILE]

The study is objects x episodes episodes (default 64 x 640 = 40,960) of the deterministic MLP
actor on held-out objects of the hard curriculum, device Philox resets, run in one process:

  host             evaluate_heldout_set(parallel=True): records and histories copied to the host,
                   episode dictionaries built, FailureClassifier.classify per episode
                   (failure_statistics.host_failure_study);
  device_history   run_failure_study(keep_history=True): the episode launch writes contact_hist,
                   dxrl_failure_summarize reduces it; only the tables cross to the host;
  device_moments   run_failure_study(keep_history=False): the episode kernel accumulates the
                   history moments, no history is allocated.

The three forms alternate within a round (one warm-up round first, then --rounds timed rounds);
per form: wall clock around the whole call, HIP-event time of the episode kernel and of the two
summary launches, and the bytes copied to the host; median, min and max over the rounds.  The
A/B of the episode kernel with and without the history writes is the pair
device_history / device_moments: same build, same lanes, same streams.  --classify-max-steps
above the loop bound makes the modes other than timeout appear.  Writes one JSON file.
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
    ap.add_argument("--objects", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=640)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--classify-max-steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3, help="the host pipeline takes seconds: fewer timed rounds")
    ap.add_argument("--config", default="hard")
    ap.add_argument("--out", default=os.path.join("profiles", "failure_study", "bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import evaluation as ev, failure_statistics as fs

    T, K, bound = a.max_episode_steps, a.episodes, a.classify_max_steps
    h = ev.HeldOutObjectSet(getattr(pkg.CurriculumConfig, a.config)(), num_heldout_objects=a.objects, seed=42)
    pol = actor()

    def host():
        tm = {}
        r = ev.Evaluator(pol, h, max_episode_steps=T).evaluate_heldout_set(
            K, seed=0, parallel=True, device_seed=0, return_episodes=True, timing=tm)
        st = fs.host_failure_study(r["all_episodes"], bound)
        rec_bytes = 4 + len(r["all_episodes"]) * (8 + 4 + 1 + 1 + T) + 4 * len(r["all_episodes"])
        return {"kernel_ms": tm["kernel_ms"], "summary_ms": 0.0, "host_bytes": rec_bytes,
                "counts": st["statistics"]["failure_counts"]}

    def device(keep_history):
        tm = {}
        out = fs.run_failure_study(pol, h, K, 0, max_episode_steps=T, classify_max_steps=bound, parallel=True,
                                   device_seed=0, keep_history=keep_history, timing=tm)
        return {"kernel_ms": tm["kernel_ms"], "summary_ms": tm["summary_ms"], "host_bytes": out["bytes_to_host"],
                "counts": out["statistics"]["failure_counts"], "tie_rows": len(out["tie_rows"])}

    forms = [("host", host, a.host_rounds), ("device_history", lambda: device(True), a.rounds),
             ("device_moments", lambda: device(False), a.rounds)]
    runs = {name: [] for name, _, _ in forms}
    for rnd in range(-1, a.rounds):  # round -1: warm-up of every form
        for name, fn, reps in forms:
            if rnd >= reps:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            r["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if rnd >= 0:
                runs[name].append(r)
                print(json.dumps({"round": rnd, "form": name, "wall_ms": round(r["wall_ms"], 3),
                                  "kernel_ms": round(r["kernel_ms"], 4), "summary_ms": round(r["summary_ms"], 4)}),
                      flush=True)

    def spread(xs):
        return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}

    out = {"study": {"objects": a.objects, "episodes_per_object": K, "max_episode_steps": T,
                     "classify_max_steps": bound, "total_episodes": a.objects * K,
                     "policy": "deterministic MLP actor", "config": a.config,
                     "device": torch.cuda.get_device_name(0)}, "forms": {}}
    for name, rs in runs.items():
        if not rs:
            continue
        out["forms"][name] = {
            "rounds": len(rs), "wall_ms": spread([r["wall_ms"] for r in rs]),
            "episode_kernel_ms": spread([r["kernel_ms"] for r in rs]),
            "summary_ms": spread([r["summary_ms"] for r in rs]),
            "host_ms": spread([r["wall_ms"] - r["kernel_ms"] - r["summary_ms"] for r in rs]),
            "host_bytes": rs[-1]["host_bytes"], "failure_counts": rs[-1]["counts"],
            **({"tie_rows": rs[-1]["tie_rows"]} if "tie_rows" in rs[-1] else {})}
    hk, mk = ([r["kernel_ms"] for r in runs[n]] for n in ("device_history", "device_moments"))
    if hk and mk:
        out["episode_kernel_ab"] = {
            "history_ms": spread(hk), "moments_ms": spread(mk),
            "moments_minus_history_ms": round(statistics.median(mk) - statistics.median(hk), 4),
            "round_spread_ms": round(max(max(hk) - min(hk), max(mk) - min(mk)), 4)}
    print(json.dumps(out["forms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
