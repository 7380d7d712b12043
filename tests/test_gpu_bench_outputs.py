"""GPU: bench.py's plain run, --dump-outputs and --full, in-process on a small workload.

A plain run reports the headline figure only; --dump-outputs writes what the last timed step
computed, identically on every run (the clock prewarm, whose iteration count depends on the
clock, runs on a twin of the workload); --full adds the figures beside the headline."""
import json
import os

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu

ENVS, HORIZON, STEPS, WARMUP = 256, 16, 2, 1
ARGS = ["--gpus", "1", "--envs", str(ENVS), "--horizon", str(HORIZON), "--steps", str(STEPS), "--warmup", str(WARMUP),
        "--prewarm-s", "0.05"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"phases_ms", "mfma", "train_stats", "device_memory_gb", "roofline", "step_kernel_at_bench_envs",
             "cpu_baseline", "rollout_kernel_ms"}


def run(capsys, *more):
    bench.main(ARGS + list(more))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_reports_the_headline_only(capsys):
    d = run(capsys)
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d)
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["unit"] == "env-steps/s" and d["higher_is_better"]
    want = ENVS * HORIZON * STEPS / (d["ms_per_step"] * 1e-3 * STEPS)
    assert abs(d["value"] - want) <= 1e-3 * want


def test_full_run_adds_the_other_figures(capsys):
    d = run(capsys, "--full", "--no-roofline", "--no-cpu-baseline")
    assert HEADLINE <= set(d) and {"phases_ms", "mfma", "train_stats", "device_memory_gb"} <= set(d)
    assert "rollout" in d["phases_ms"] and d["train_stats"]["prewarm"]["iterations"] >= 8


def test_dumped_outputs_are_the_last_timed_step_and_repeat(capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run(capsys, "--dump-outputs", a)
    run(capsys, "--dump-outputs", b, "--prewarm-s", "0.3")  # more prewarm iterations: the same files
    A, B = load(a), load(b)
    assert set(A) == set(B) == {"params", "obs", "act", "logp", "rew", "done", "values", "adv", "ret"}
    assert sum(x.nbytes for x in A.values()) <= 64e6
    for k in A:
        assert A[k].dtype in (np.float32, np.float64) and np.isfinite(A[k]).all(), k
        assert np.array_equal(A[k], B[k]), k
    # the same workload driven directly for W + K iterations leaves exactly these arrays
    from dexterous_rl_manipulation_amd.workloads import build_pg_workload
    _, tr = build_pg_workload("easy", torch.device("cuda", 0), envs=ENVS, horizon=HORIZON)
    for _ in range(WARMUP + STEPS):
        tr.iteration()
    torch.cuda.synchronize()
    assert A["act"].shape == (ENVS * HORIZON, tr.act.shape[1]) and A["obs"].shape[0] == ENVS * (HORIZON + 1)
    for k, t in (("params", tr.params), ("act", tr.act), ("rew", tr.rew), ("adv", tr.adv), ("values", tr.V[0]),
                 ("obs", tr.obs_rm), ("done", tr.done)):
        assert np.array_equal(A[k], t.float().cpu().numpy()), k


def test_simple_learner_outputs_repeat(capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        run(capsys, "--learner", "simple", "--dump-outputs", d)
    A, B = load(a), load(b)
    assert set(A) == {"mean_action", "best_reward", "episode_return", "joint_positions", "object_position"}
    for k in A:
        assert A[k].dtype in (np.float32, np.float64) and np.array_equal(A[k], B[k], equal_nan=True), k
