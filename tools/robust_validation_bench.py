"""What a noise-level validation costs inside a training run (config_easy, 4096 envs x 200 steps, a
validation of 64 held-out objects x 10 episodes of at most 200 steps under every level of
ValidationPlan.sweep_levels([0, .01, .05, .1], [0, .01, .05, .1]) every 10 iterations).

Arms on one trainer, alternated over repeats, each timed by the host clock around work that ends
in a device synchronise and by device events:
  a  fit(iters)                                                  (no validation)
  b  fit(iters, validation=levels plan, validate_every=10,       (the plan built once, the three
         val_keep_best="worst_success_rate")                      tables on the device)
  c  fit(10) + tr.policy() + RobustnessTester(policy, config_easy).robustness_study(the same noise
     lists, objects x episodes episodes per level, parallel=True), repeated
                                                                 (the host loop b replaces: a
     snapshot, a new env, plan and launch, one summarise call and a synchronise per validation;
     it runs the reference's level list with its repeats and has no per-object tables)
and the validation alone: plan.run (episode kernel + dxrl_pg_val_levels_row) back to back, device
events.  Prints one JSON line: ms per iteration per arm (median, min, max over repeats).

    python tools/robust_validation_bench.py [--iters 30] [--repeats 7] [--out FILE]
    python tools/robust_validation_bench.py --profile   # a short validated fit for rocprofv3 --kernel-trace --stats

--common-random-numbers is another arm of its own (with --profile: the validated fit runs the plan
built with common_random_numbers=True).  On one trainer it alternates, over the repeats, plan.run
back to back for the levels plan without and with common random numbers (device events), then
runs fit(--paired-iters, validation=the CRN plan) and prints, for the last validation's weights
and every level, return_diff_std and paired_degradation_stderr from the device's paired table
beside the same formulas applied on the host to the records of the plan without common random
numbers (independent episodes per level): the variance reduction the pairing buys.

--failure-modes is another arm of its own (with --profile: the validated fit runs the levels plan
with common random numbers and failure_modes=True).  On one trainer it alternates, over the
repeats, plan.run back to back for the CRN levels plan without and with failure_modes (device
events), then fit(--iters, validate_every=--every) with each of the two plans (host clock and
device events), and prints the last validation's dominant mode per level.  A commit that has no
failure_modes option (the parent of the one that added it) runs the arms it has.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OBS_LEVELS = [0.0, 0.01, 0.05, 0.1]
DYN_LEVELS = [0.0, 0.01, 0.05, 0.1]


def host_paired(ret0, ret1, suc0, suc1):
    """return_diff_std and paired_degradation_stderr (include/dxrl.h's definitions) of two record
    sets on the host."""
    d = ret1 - ret0
    n = d.size
    lost, gained = int(((suc0 != 0) & (suc1 == 0)).sum()), int(((suc0 == 0) & (suc1 != 0)).sum())
    v = max(((lost + gained) - (lost - gained) ** 2 / n) / n, 0.0)
    return {"mean_return_diff": float(d.mean()), "return_diff_std": float(d.std()),
            "paired_degradation": (lost - gained) / n, "paired_degradation_stderr": v ** 0.5 / n ** 0.5}


def paired_arm(a, tr, plan, crn, score, torch):
    from dexterous_rl_manipulation_amd import training_run as run
    tr.fit(a.warmup)
    arms = {"levels": (plan, run._ValState(tr, plan.fingerprint, plan.object_names)),
            "levels_crn": (crn, run._ValState(tr, crn.fingerprint, crn.object_names))}
    for pl, val in arms.values():
        pl.run(tr, val, 0, 0, 0)
    torch.cuda.synchronize()
    alone = {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, (pl, val) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            val.rows = 0  # the tables are scratch here
            e0.record()
            for _ in range(10):
                pl.run(tr, val, 0, 0, 0)
            e1.record()
            e1.synchronize()
            alone[name].append(e0.elapsed_time(e1) / 10)
    log = tr.fit(a.paired_iters, validation=crn, validate_every=a.every, val_keep_best=score)
    v = log.validation
    pl, val = arms["levels"]
    val.rows = 0
    pl.run(tr, val, 0, 0, 0)  # independent episodes per level, on the weights of the last validation
    torch.cuda.synchronize()
    ret, suc = pl.ep_return.cpu().numpy(), pl.ep_success.cpu().numpy()
    n = pl.G * pl.K
    per_level = []
    for l, (o, d) in enumerate(crn.noise_levels):
        s = slice(l * n, (l + 1) * n)
        row = {"obs_noise_std": o, "dyn_noise_std": d,
               "success_rate_crn": float(v.level_column("success_rate")[-1, l]),
               "success_rate_independent": float((suc[s] != 0).mean()),
               "crn": {k: float(v.paired_column(k)[-1, l]) for k in ("mean_return_diff", "return_diff_std",
                                                                      "paired_degradation",
                                                                      "paired_degradation_stderr", "lost", "gained")},
               "independent": host_paired(ret[:n], ret[s], suc[:n], suc[s])}
        per_level.append(row)
    res = {"envs": a.envs, "horizon": a.horizon, "paired_iters": a.paired_iters, "validate_every": a.every,
           "repeats": a.repeats, "objects": a.objects, "episodes_per_object": a.episodes,
           "noise_levels": [list(x) for x in crn.noise_levels], "pairs_per_level": n,
           "validations": len(v), "device": torch.cuda.get_device_name(tr.dev), "per_level_last_row": per_level}
    for name, t in alone.items():
        res[f"validation_alone_ms_{name}"] = {"median": statistics.median(t), "min": min(t), "max": max(t), "all": t}
    return res


def failure_arm(a, tr, crn, with_modes, score, torch):
    from dexterous_rl_manipulation_amd import training_run as run
    tr.fit(a.warmup)
    plans = {"crn": crn}
    if with_modes is not None:
        plans["crn_failure_modes"] = with_modes
    arms = {k: (pl, run._ValState(tr, pl.fingerprint, pl.object_names)) for k, pl in plans.items()}
    for pl, val in arms.values():
        pl.run(tr, val, 0, 0, 0)
    torch.cuda.synchronize()
    alone = {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, (pl, val) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            val.rows = 0  # the tables are scratch here
            e0.record()
            for _ in range(10):
                pl.run(tr, val, 0, 0, 0)
            e1.record()
            e1.synchronize()
            alone[name].append(e0.elapsed_time(e1) / 10)
    # fit per iteration with the levels validation in both settings: one trainer per plan (a run's
    # validation table belongs to one plan), alternated
    from dexterous_rl_manipulation_amd import workloads
    fits, wall, events = {}, {k: [] for k in plans}, {k: [] for k in plans}
    for name, pl in plans.items():
        _, t = workloads.build_pg_workload("easy", tr.dev, envs=a.envs, horizon=a.horizon)
        kw = {} if name == "crn" else dict(failure_modes=True)
        fits[name] = (t, t.validation_plan(a.heldout, episodes_per_object=a.episodes, seed=0, device_seed=0,
                                           noise_levels=crn.noise_levels, common_random_numbers=True, **kw))
        t.fit(a.warmup, validation=fits[name][1], validate_every=a.every, val_keep_best=score)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, (t, pl) in fits.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            log = t.fit(a.iters, validation=pl, validate_every=a.every, val_keep_best=score)
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
            events[name].append(e0.elapsed_time(e1) / a.iters)
    res = {"envs": a.envs, "horizon": a.horizon, "iters": a.iters, "validate_every": a.every, "repeats": a.repeats,
           "objects": a.objects, "episodes_per_object": a.episodes, "levels": len(crn.noise_levels),
           "validation_episodes": crn.E, "device": torch.cuda.get_device_name(tr.dev)}
    for name in plans:
        t, w, e = alone[name], wall[name], events[name]
        res[f"validation_alone_ms_{name}"] = {"median": statistics.median(t), "min": min(t), "max": max(t), "all": t}
        res[f"fit_{name}"] = {"wall_ms_per_iteration_median": statistics.median(w), "min": min(w), "max": max(w),
                              "all": w, "event_ms_per_iteration_median": statistics.median(e)}
    if with_modes is not None:
        res["failure_modes_minus_crn_us_per_validation"] = 1e3 * (
            res["validation_alone_ms_crn_failure_modes"]["median"] - res["validation_alone_ms_crn"]["median"])
        v = log.validation
        res["last_row"] = {"dominant_mode": v.statistics()["final_dominant_failure_mode"],
                           "dominant_frequency": v.statistics()["final_dominant_failure_frequency"],
                           "failure_rate": v.statistics()["final_failure_rate"],
                           "lost_into_mode_worst_level": v.failure_transitions[-1, -1, 0].tolist()}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--every", type=int, default=10)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--horizon", type=int, default=200)
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--episodes", type=int, default=10)
    p.add_argument("--out", default=None)
    p.add_argument("--profile", action="store_true")
    p.add_argument("--common-random-numbers", action="store_true")
    p.add_argument("--paired-iters", type=int, default=200)
    p.add_argument("--failure-modes", action="store_true")
    a = p.parse_args()
    import torch
    from dexterous_rl_manipulation_amd import CurriculumConfig, workloads
    from dexterous_rl_manipulation_amd.evaluation import HeldOutObjectSet
    from dexterous_rl_manipulation_amd.evaluator import RobustnessTester
    from dexterous_rl_manipulation_amd.training_run import ValidationPlan
    dev = torch.device("cuda", 0)
    env, tr = workloads.build_pg_workload("easy", dev, envs=a.envs, horizon=a.horizon)
    heldout = HeldOutObjectSet(CurriculumConfig.easy(), num_heldout_objects=a.objects)
    levels = ValidationPlan.sweep_levels(OBS_LEVELS, DYN_LEVELS)
    plan = tr.validation_plan(heldout, episodes_per_object=a.episodes, seed=0, device_seed=0, noise_levels=levels)
    score = "worst_success_rate"
    crn = None
    if a.common_random_numbers or a.failure_modes:
        crn = tr.validation_plan(heldout, episodes_per_object=a.episodes, seed=0, device_seed=0, noise_levels=levels,
                                 common_random_numbers=True)
    with_modes = None
    if a.failure_modes and "failure_modes" in ValidationPlan.__init__.__code__.co_varnames:
        with_modes = tr.validation_plan(heldout, episodes_per_object=a.episodes, seed=0, device_seed=0,
                                        noise_levels=levels, common_random_numbers=True, failure_modes=True)
    if a.profile:
        tr.fit(a.iters, validation=with_modes or crn or plan, validate_every=a.every, val_keep_best=score)
        torch.cuda.synchronize()
        return
    if crn is not None:
        a.heldout = heldout
        arm = failure_arm(a, tr, crn, with_modes, score, torch) if a.failure_modes else \
            paired_arm(a, tr, plan, crn, score, torch)
        line = json.dumps(arm)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return

    def plain():
        tr.fit(a.iters)

    def validated():
        tr.fit(a.iters, validation=plan, validate_every=a.every, val_keep_best=score)

    def host_loop():
        for _ in range(a.iters // a.every):
            tr.fit(a.every)
            rt = RobustnessTester(tr.policy(), CurriculumConfig.easy(), max_episode_steps=env.max_episode_steps,
                                  device=dev)
            rt.robustness_study(OBS_LEVELS, DYN_LEVELS, a.objects * a.episodes, 0, parallel=True, device_seed=0)

    arms = {"a_fit": plain, "b_fit_levels_validation": validated, "c_fit_host_robustness_study": host_loop}
    tr.fit(a.warmup)
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    wall = {k: [] for k in arms}
    events = {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
            events[name].append(e0.elapsed_time(e1) / a.iters)
    # the validation alone: episode kernel + levels row, back to back on the trainer's weights
    val = tr._run.val
    alone = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            plan.run(tr, val, 0, 0, 0)
        e1.record()
        e1.synchronize()
        alone.append(e0.elapsed_time(e1) / 10)
    res = {"envs": a.envs, "horizon": a.horizon, "iters": a.iters, "validate_every": a.every, "repeats": a.repeats,
           "objects": a.objects, "episodes_per_object": a.episodes, "noise_levels": [list(x) for x in levels],
           "validation_episodes": len(levels) * a.objects * a.episodes,
           "host_loop_levels": len(RobustnessTester.sweep_levels(OBS_LEVELS, DYN_LEVELS)[0]),
           "validations_per_run": a.iters // a.every, "device": torch.cuda.get_device_name(dev)}
    for name in arms:
        v, e = wall[name], events[name]
        res[name] = {"wall_ms_per_iteration_median": statistics.median(v), "min": min(v), "max": max(v), "all": v,
                     "event_ms_per_iteration_median": statistics.median(e)}
    med = lambda k: res[k]["wall_ms_per_iteration_median"]  # noqa: E731
    per_val = a.iters / max(1, a.iters // a.every)
    res["b_minus_a_ms_per_validation"] = (med("b_fit_levels_validation") - med("a_fit")) * per_val
    res["c_minus_a_ms_per_validation"] = (med("c_fit_host_robustness_study") - med("a_fit")) * per_val
    res["a_spread_ms_per_iteration"] = res["a_fit"]["max"] - res["a_fit"]["min"]
    res["validation_alone_ms"] = {"median": statistics.median(alone), "min": min(alone), "max": max(alone)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
