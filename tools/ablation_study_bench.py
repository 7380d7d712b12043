"""The two training studies with their runs summarised on the host and on the device.

    python tools/ablation_study_bench.py [--runs-per-arm 4096] [--episodes 200] [--max-episode-steps 200]
                                         [--component-seeds 1024] [--rounds 3] [--out FILE]

Curriculum study (curriculum_ablation.run_ablation_study): 2 arms x --runs-per-arm runs x --episodes
episodes, Philox streams, success_rule="terminated", in one process:

  host    device_summary=False: train_runs copies every episode record, replays every lane's
          scheduler on the host and calls compute_convergence_metrics / aggregate_metrics per run;
  device  device_summary=True: the launch, dxrl_study_summarize, medians from the lane table.

Component study (ablation.run_component_study): 4 configurations x --component-seeds seeds, same
streams and success rule, device_summary=True against device_summary=False (the records copied
and summarised run by run as run_component_ablation does).

The forms alternate within a round (one warm-up round at a sixteenth of the size first, then
--rounds timed rounds).  Per form: wall clock around the whole call, HIP-event time of the rollout
launches and of the summary launches, and the bytes copied to the host.  The lane pass and the
group pass are also timed apart (HIP events, seven repeats on one launched study).  Writes one
JSON file; nothing is asserted about which form is faster.
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs-per-arm", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--component-seeds", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "ablation_study", "bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from dexterous_rl_manipulation_amd import _native as N, ablation as A, curriculum_ablation as CA

    E, T = a.episodes, a.max_episode_steps
    last = {"rollout": [], "summary_ms": 0.0}

    real_launch = CA.DeviceStudy.launch

    def launch(self, *args, **kw):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(torch.cuda.current_stream(self.device))
        real_launch(self, *args, **kw)
        t1.record(torch.cuda.current_stream(self.device))
        last["rollout"].append((t0, t1))

    real_summarize = CA.summarize_runs

    def summarize(*args, **kw):
        tm = {}
        out = real_summarize(*args, timing=tm, **kw)
        last["summary_ms"] = tm["summary_ms"]
        return out

    CA.DeviceStudy.launch = launch
    CA.summarize_runs = summarize

    def curriculum(device_summary, runs):
        with contextlib.redirect_stdout(io.StringIO()), tempfile_dir() as d:
            return CA.run_ablation_study(num_episodes=E, num_runs=runs, output_dir=d, success_rule="terminated",
                                         device_streams=True, device_summary=device_summary)

    def component(device_summary, seeds):
        with contextlib.redirect_stdout(io.StringIO()):
            return A.run_component_study(E, T, list(range(1000, 1000 + seeds)), success_rule="terminated",
                                         device_streams=True, device_summary=device_summary)

    def timed(fn, *args):
        last["rollout"], last["summary_ms"] = [], 0.0
        CA.BYTES_COPIED["records"] = CA.BYTES_COPIED["summary"] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(*args)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        device_form = args[0]
        return res, {"wall_ms": wall, "rollout_ms": max(x.elapsed_time(y) for x, y in last["rollout"]),
                     "summary_ms": last["summary_ms"] if device_form else 0.0,
                     "host_bytes": CA.BYTES_COPIED["summary" if device_form else "records"]}

    def spread(xs):
        return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}

    out = {"device": torch.cuda.get_device_name(0), "episodes": E, "max_episode_steps": T, "studies": {}}
    for study, fn, size in (("curriculum", curriculum, a.runs_per_arm), ("component", component, a.component_seeds)):
        runs = {"host": [], "device": []}
        results = {}
        for rnd in range(-1, a.rounds):
            for form, dev_form in (("host", False), ("device", True)):
                res, r = timed(fn, dev_form, max(size // 16, 2) if rnd < 0 else size)
                results[form] = res
                if rnd >= 0:
                    runs[form].append(r)
                    print(json.dumps({"study": study, "round": rnd, "form": form,
                                      **{k: round(v, 3) for k, v in r.items()}}), flush=True)
        lanes = (2 if study == "curriculum" else 4) * size
        entry = {"lanes": lanes, "rounds": a.rounds,
                 "max_relative_difference": max_rel(json.loads(json.dumps(results["host"])),
                                                    json.loads(json.dumps(results["device"]))),
                 "forms": {}}
        for form, rs in runs.items():
            entry["forms"][form] = {
                "wall_ms": spread([r["wall_ms"] for r in rs]), "rollout_ms": spread([r["rollout_ms"] for r in rs]),
                "summary_ms": spread([r["summary_ms"] for r in rs]),
                "host_ms": spread([r["wall_ms"] - r["rollout_ms"] - r["summary_ms"] for r in rs]),
                "host_bytes": rs[-1]["host_bytes"]}
        out["studies"][study] = entry

    # the two kernels apart, on one launched curriculum study
    CA.DeviceStudy.launch = real_launch
    sched, hard = CA.reference_scheduler(), CA.CurriculumConfig.hard()
    n = a.runs_per_arm
    jobs = [(sched, 42 + r) for r in range(n)] + [(hard, 42 + r) for r in range(n)]
    st = CA.launch_runs(jobs, E, T, success_rule="terminated", device_streams=True)
    try:
        dev, L = st.device, st.n
        t = {k: torch.zeros(s, dtype=d, device=dev) for k, s, d in (
            ("li", (L, 8), torch.int64), ("lr", (L, 4), torch.float64), ("gs", (3, 16), torch.int64),
            ("gm", (3, 5, 3), torch.float64), ("tie", (1 + L,), torch.int32), ("status", (1,), torch.int32))}
        off = torch.tensor([0, n, 2 * n, 4 * n], dtype=torch.int32, device=dev)
        mem = torch.cat([torch.arange(2 * n), torch.arange(2 * n)]).to(torch.int32).to(dev)

        def call(lanes, groups):
            s = N.StudySummaryArgs()
            s.num_lanes, s.record_cap, s.lane_offset, s.total_lanes = (L if lanes else 0), st.record_cap, 0, L
            s.window, s.min_count, s.reward_threshold = 20, CA.min_successes(20, 0.5), 0.5
            s.ep_return, s.ep_length, s.ep_success = N.ptr(st.ep_return), N.ptr(st.ep_length), N.ptr(st.ep_success)
            s.ep_level, s.lane_episodes = N.ptr(st.ep_level), N.ptr(st.ep_count)
            s.lane_ints, s.lane_reals, s.status = N.ptr(t["li"]), N.ptr(t["lr"]), N.ptr(t["status"])
            if groups:
                s.num_groups, s.num_members, s.tie_cap = 3, 4 * n, L
                s.group_offsets, s.group_lanes = N.ptr(off), N.ptr(mem)
                s.group_stats, s.group_metrics = N.ptr(t["gs"]), N.ptr(t["gm"])
                s.tie_count, s.tie_list = N.ptr(t["tie"]), N.ptr(t["tie"][1:])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            N.call("dxrl_study_summarize", dev.index, C.byref(s), N.stream_of(dev))
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        call(True, True)
        out["kernels"] = {"lanes": L, "groups": 3,
                          "lane_pass_ms": spread([call(True, False) for _ in range(7)]),
                          "group_pass_ms": spread([call(False, True) for _ in range(7)]),
                          "record_bytes": L * st.record_cap * (8 + 4 + 1 + 4),
                          "lane_table_bytes": L * (8 * 8 + 4 * 8)}
    finally:
        st.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


def max_rel(a, b):
    """Largest relative difference between two nested results (inf where they differ otherwise)."""
    if isinstance(a, dict) and isinstance(b, dict) and set(a) == set(b):
        return max([max_rel(a[k], b[k]) for k in a], default=0.0)
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return max([max_rel(x, y) for x, y in zip(a, b)], default=0.0)
    if isinstance(a, float) and isinstance(b, float):
        if a == b or (a != a and b != b):
            return 0.0
        return abs(a - b) / max(abs(a), abs(b))
    return 0.0 if a == b else float("inf")


@contextlib.contextmanager
def tempfile_dir():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        yield d


if __name__ == "__main__":
    main()
