"""Host share of a seed-variance study with and without the device episode summary.

    python tools/seed_variance_bench.py [--seeds 64] [--objects 64] [--episodes 10]
                                        [--max-episode-steps 200] [--repeats 3] [--out FILE]

The study is seeds x objects x episodes episodes (default 64 x 64 x 10 = 40,960) of the
deterministic MLP actor, device Philox resets, run in one process:

  per_seed_host     one evaluate_heldout_set(parallel=True, return_episodes=False) per seed, the
                    summaries on the host (records and contact_hist copied back);
  per_seed_device   the same calls with device_summary=True (dxrl_eval_summarize);
  one_launch        SeedVarianceAnalyzer.evaluate_multiple_seeds(parallel=True): one episode launch
                    and one summary launch for the whole study;
  one_call_host /   the same episode count as ONE evaluate_heldout_set (objects x seeds*episodes),
  one_call_device   host summaries against device summaries at the full E x max_steps.

Per form: wall clock around the whole call (device idle before and after), the HIP-event time of
the episode kernel(s) and of the two summary launches, and the bytes copied to the host.  One
warm-up run, then --repeats timed runs; median, min and max are reported.  Writes one JSON file.
"""
import argparse
import contextlib
import io
import json
import math
import os
import statistics
import sys
import time


def actor():
    """The trainer's initialisation of the MLP actor (orthogonal, head gain 2), deterministic."""
    import torch
    from dexterous_rl_manipulation_amd.policies import MLPActorPolicy
    g = torch.Generator(device="cpu").manual_seed(0)
    w = {}
    for name, rows, cols, gain in (("W1a", 256, 45, math.sqrt(2)), ("W2a", 256, 256, math.sqrt(2)),
                                   ("W3a", 15, 256, 2.0)):
        w[name] = torch.empty(rows, cols)
        torch.nn.init.orthogonal_(w[name], gain=gain, generator=g)
    W1, W2, W3 = torch.zeros(256, 64), torch.zeros(256, 288), torch.zeros(32, 288)
    W1[:, :45], W2[:, :256], W3[:15, :256] = w["W1a"], w["W2a"], w["W3a"]
    return MLPActorPolicy(W1, W2, W3, torch.full((15,), -0.5), deterministic=True, seed=0)


def record_bytes(rec) -> int:
    return 4 + sum(x.nbytes for x in (rec.ep_return, rec.ep_length, rec.ep_contacts, rec.contact_hist,
                                      rec.policy_used)) + len(rec.ep_success)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--objects", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one-call-repeats", type=int, default=2)
    ap.add_argument("--config", default="variable")
    ap.add_argument("--out", default=os.path.join("profiles", "seed_variance", "bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import evaluation as ev, seed_variance as sv

    T, K = a.max_episode_steps, a.episodes
    seeds = [1000 + 7 * i for i in range(a.seeds)]
    h = ev.HeldOutObjectSet(getattr(pkg.CurriculumConfig, a.config)(), num_heldout_objects=a.objects, seed=42)
    pol = actor()

    def per_seed(device_summary):
        t = {"kernel_ms": 0.0, "summary_ms": 0.0, "host_bytes": 0, "success": []}
        for s in seeds:
            tm = {}
            r = ev.Evaluator(pol, h, max_episode_steps=T).evaluate_heldout_set(
                K, seed=s, parallel=True, device_seed=s, return_episodes=False, device_summary=device_summary,
                timing=tm)
            t["kernel_ms"] += tm["kernel_ms"]
            t["summary_ms"] += tm.get("summary_ms", 0.0)
            t["host_bytes"] += r["summary"].host_bytes if device_summary else record_bytes(r["records"])
            t["success"].append(r["metrics"]["grasp_success_rate"])
        return t

    def one_launch():
        an = sv.SeedVarianceAnalyzer(pol, h, "dense", T)
        tm = {}
        with contextlib.redirect_stdout(io.StringIO()):
            res = an.evaluate_multiple_seeds(seeds, K, parallel=True, device_seed=0, timing=tm)
        return {"kernel_ms": tm["kernel_ms"], "summary_ms": tm["summary_ms"],
                "host_bytes": an.last_summary.host_bytes,
                "success": [res[s]["metrics"]["grasp_success_rate"] for s in seeds]}

    def one_call(device_summary):
        tm = {}
        r = ev.Evaluator(pol, h, max_episode_steps=T).evaluate_heldout_set(
            K * len(seeds), seed=0, parallel=True, device_seed=0, return_episodes=False,
            device_summary=device_summary, timing=tm)
        return {"kernel_ms": tm["kernel_ms"], "summary_ms": tm.get("summary_ms", 0.0),
                "host_bytes": r["summary"].host_bytes if device_summary else record_bytes(r["records"]),
                "success": [r["metrics"]["grasp_success_rate"]]}

    forms = [("per_seed_host", lambda: per_seed(False), a.repeats),
             ("per_seed_device", lambda: per_seed(True), a.repeats), ("one_launch", one_launch, a.repeats),
             ("one_call_host", lambda: one_call(False), a.one_call_repeats),
             ("one_call_device", lambda: one_call(True), a.one_call_repeats)]
    out = {"study": {"seeds": a.seeds, "objects": a.objects, "episodes_per_object": K, "max_episode_steps": T,
                     "total_episodes": a.seeds * a.objects * K, "policy": "deterministic MLP actor",
                     "config": a.config, "device": torch.cuda.get_device_name(0)}, "forms": {}}
    for name, fn, reps in forms:
        if reps <= 0:
            continue
        fn()  # warm-up
        wall, runs = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            runs.append(r)

        def spread(xs):
            return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}

        kern, summ = [r["kernel_ms"] for r in runs], [r["summary_ms"] for r in runs]
        out["forms"][name] = {
            "repeats": reps, "wall_ms": spread(wall), "episode_kernel_ms": spread(kern), "summary_ms": spread(summ),
            "host_ms": spread([w - k - s for w, k, s in zip(wall, kern, summ)]),
            "host_bytes": runs[-1]["host_bytes"],
            "mean_success_rate": sum(runs[-1]["success"]) / len(runs[-1]["success"])}
        print(json.dumps({name: out["forms"][name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
