"""GPU checks of the studies built on dxrl_study_summarize: ablation.run_component_study /
train_study / the command line (the reference's own runs of tests/golden/eval_golden.json
"ablation"; schedulers that move, against the CPU oracle composition of
tests/curriculum_reference.py) and curriculum_ablation.run_ablation_study(device_summary=True)
(tests/golden/curriculum_golden.json "study"; both modes on one Philox study)."""
import functools
import json

import numpy as np
import pytest

from dexterous_rl_manipulation_amd import ablation as A
from dexterous_rl_manipulation_amd import curriculum_ablation as CA
from dexterous_rl_manipulation_amd.experiments import (CurriculumConfig, CurriculumScheduler,
                                                       CurriculumSchedulerConfig, load_named_config)

import curriculum_reference as R
import study_summary_reference as S
from test_curriculum_study_host import golden as curriculum_golden
from test_eval_host import golden as eval_golden

pytestmark = pytest.mark.gpu

RTOL = 1e-12  # the project's bound for f64 episode returns


def check(res, want):
    """test_gpu_ablation.check, restated."""
    got = res.to_dict()
    assert got["episode_steps"] == want["episode_steps"]
    assert got["success_rates"] == want["success_rates"]
    np.testing.assert_allclose(got["episode_rewards"], want["episode_rewards"], rtol=1e-12, atol=1e-15)
    for k in ("final_success_rate", "mean_episode_length", "convergence_step", "total_episodes", "config"):
        assert got[k] == want[k], k


def close(got, want, path=""):
    """test_gpu_curriculum_study.close, restated: nested equality; floats to RTOL."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), path
        for k in want:
            close(got[k], want[k], f"{path}.{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), path
        for i, (a, b) in enumerate(zip(got, want)):
            close(a, b, f"{path}[{i}]")
    elif isinstance(want, float):
        assert got == pytest.approx(want, rel=RTOL, abs=1e-15), path
    else:
        assert got == want, path


def stats_close(got, want):
    assert set(got) == set(want)
    for name, groups in want.items():
        for grp, d in groups.items():
            for k, v in d.items():
                if isinstance(v, float):
                    assert got[name][grp][k] == pytest.approx(v, rel=1e-12), (name, grp, k)
                else:
                    assert got[name][grp][k] == v, (name, grp, k)


# ------------------------------------------------------------------ 1. the reference's own runs
def test_run_component_study_matches_reference(tmp_path):
    g = eval_golden()["ablation"]
    env_seeds = {(r["name"], r["seed"]): r["env_seed"] for r in g["runs"]}
    stats, runs = A.run_component_study(num_episodes=g["num_episodes"], max_episode_steps=g["max_episode_steps"],
                                        seeds=[42, 123], success_rule="training", env_seeds=env_seeds,
                                        return_runs=True, output_dir=str(tmp_path))
    stats_close(stats, g["statistics"])
    for r in g["runs"]:
        check(runs[r["name"]][[42, 123].index(r["seed"])], r["result"])
    saved = json.load(open(tmp_path / "component_ablation_results.json"))
    assert list(saved) == [nm for nm, _, _ in A.ABLATION_CONFIGS] and len(saved["baseline"]) == 2
    only = A.run_component_study(num_episodes=g["num_episodes"], max_episode_steps=g["max_episode_steps"],
                                 seeds=[42, 123], env_seeds=env_seeds)
    assert only == stats
    host = A.run_component_study(num_episodes=g["num_episodes"], max_episode_steps=g["max_episode_steps"],
                                 seeds=[42, 123], env_seeds=env_seeds, device_summary=False)
    stats_close(host, g["statistics"])


def test_run_ablation_study_device_summary_matches_reference(tmp_path, capsys):
    g = curriculum_golden()["study"]
    res = CA.run_ablation_study(num_episodes=g["num_episodes"], num_runs=g["num_runs"], output_dir=str(tmp_path),
                                env_seeds=g["env_seeds_with"] + g["env_seeds_without"], device_summary=True)
    close(json.loads(json.dumps(res)), g["result"])
    close(json.load(open(tmp_path / "curriculum_ablation.json")), g["saved"])
    assert capsys.readouterr().out.replace(str(tmp_path), "<output_dir>") == g["report"]


# ------------------------------------------------------------------ 2. schedulers that move
SEEDS, EPISODES, MAX_STEPS = [42, 123, 456, 789], 70, 50
SCHED = CurriculumSchedulerConfig(success_rate_threshold=0.3, window_size=15, min_episodes_before_progression=20,
                                  progression_steps=5)


def env_seed_of(name, seed):
    return 5000 + seed + 17 * [nm for nm, _, _ in A.ABLATION_CONFIGS].index(name)


@functools.lru_cache(None)
def oracle_study(threshold=0.3):
    """{name: [(rewards, steps, successes, levels) per seed]} from the CPU oracle composition; a
    fixed-hard arm is a hard -> hard scheduler that cannot progress (the oracle takes schedulers)."""
    cfg = CurriculumSchedulerConfig(success_rate_threshold=threshold, window_size=15,
                                    min_episodes_before_progression=20, progression_steps=5)
    out = {}
    for name, cur, dense in A.ABLATION_CONFIGS:
        proto = A.study_scheduler(cfg) if cur else CurriculumScheduler(
            CurriculumConfig.hard(), CurriculumConfig.hard(), success_rate_threshold=2.0, window_size=15,
            min_episodes_before_progression=20, progression_steps=5)
        out[name] = [R.curriculum_run(proto, s, env_seed_of(name, s), EPISODES, MAX_STEPS, dense) for s in SEEDS]
    return out


def oracle_results(want):
    return {name: [A._summarise(A.AblationConfig(cur, dense, name), np.asarray(w[0]), np.asarray(w[1]),
                                np.asarray(w[2], dtype=bool), EPISODES) for w in want[name]]
            for name, cur, dense in A.ABLATION_CONFIGS}


def test_moving_schedulers_match_oracle():
    want = oracle_study()
    ref = oracle_results(want)
    # the expected tables are not degenerate: rates differ between arms, some runs converge, the curriculum moves
    finals = {name: [r.final_success_rate for r in rs] for name, rs in ref.items()}
    assert len({x for v in finals.values() for x in v}) >= 2 and len({tuple(v) for v in finals.values()}) >= 2
    assert any(r.convergence_step is not None for rs in ref.values() for r in rs)
    assert all(w[3][-1] > 0.0 for w in want["baseline"])
    jobs = [(A.AblationConfig(cur, dense, name), s) for name, cur, dense in A.ABLATION_CONFIGS for s in SEEDS]
    studies, lane = A.train_study(jobs, EPISODES, MAX_STEPS, curriculum_scheduler_config=SCHED,
                                  success_rule="terminated", env_seeds=[env_seed_of(c.name, s) for c, s in jobs])
    try:
        groups = {name: [lane[k] for k, (c, _) in enumerate(jobs) if c.name == name] for name, _, _ in A.ABLATION_CONFIGS}
        out = CA.summarize_runs(studies, groups, return_runs=True)
        levels = A.study_scheduler(SCHED)
        table = CA.level_table(levels)[0]
        for k, (c, s) in enumerate(jobs):
            w = ref[c.name][SEEDS.index(s)]
            row = out["lane_ints"][lane[k]]
            assert row[S.EPISODES] == EPISODES and row[S.STEPS] == sum(w.episode_steps), k
            assert row[S.FINAL_WINDOW] / 20 == w.final_success_rate, k
            assert row[S.STEPS] / EPISODES == w.mean_episode_length, k
            assert (None if row[S.CONV] < 0 else int(row[S.CONV])) == w.convergence_step, k
            assert row[S.SUCCESSES] == int(sum(w.success_rates)), k
            assert table[int(row[S.LEVEL])] == want[c.name][SEEDS.index(s)][3][-1] if c.use_curriculum \
                else row[S.LEVEL] == 0, k
            m = CA.compute_convergence_metrics(w.episode_rewards, w.success_rates)
            assert out["runs"][lane[k]]["convergence_episode"] == m["convergence_episode"]
            assert out["runs"][lane[k]]["mean_reward"] == pytest.approx(m["mean_reward"], rel=1e-12)
        assert out["tie_lanes"] == []
        stats_close(out["statistics"], A.compute_ablation_statistics(ref))
    finally:
        for st in studies:
            st.close()


def test_threshold_zero_moves_and_train_many_still_raises():
    cfg = CurriculumSchedulerConfig(success_rate_threshold=0.0, window_size=15, min_episodes_before_progression=20,
                                    progression_steps=5)
    with pytest.raises(ValueError, match="never progresses"):
        A.train_many([(A.AblationConfig(True, True, "baseline"), 42)], 5, 20, curriculum_scheduler_config=cfg)
    proto = A.study_scheduler(cfg)
    job = (A.AblationConfig(True, True, "baseline"), 42)
    want = R.curriculum_run(proto, 42, 77, 40, 30, True, success_rule="training")
    assert want[3][-1] == 1.0 and not any(want[2])  # no success reported, yet the scheduler reaches the target
    studies, lane = A.train_study([job], 40, 30, curriculum_scheduler_config=cfg, success_rule="training", env_seeds=[77])
    try:
        out = CA.summarize_runs(studies, {"baseline": lane})
        row = out["lane_ints"][0]
        assert CA.level_table(proto)[0][int(row[S.LEVEL])] == 1.0
        assert row[S.STEPS] == sum(want[1]) and row[S.SUCCESSES] == 0
        assert out["lane_reals"][0, 1] == pytest.approx(np.mean(want[0]), rel=1e-12)
    finally:
        for st in studies:
            st.close()


# ------------------------------------------------------------------ 3. both modes, one Philox study
def test_device_summary_equals_host_metrics_on_a_philox_study(tmp_path, capsys):
    kw = dict(num_episodes=60, num_runs=6, success_rule="terminated", device_streams=True)
    host = CA.run_ablation_study(output_dir=str(tmp_path / "host"), **kw)
    records = CA.BYTES_COPIED["records"]
    text = capsys.readouterr().out.replace(str(tmp_path / "host"), "<d>")
    dev = CA.run_ablation_study(output_dir=str(tmp_path / "dev"), device_summary=True, **kw)
    assert capsys.readouterr().out.replace(str(tmp_path / "dev"), "<d>") == text
    close(json.loads(json.dumps(dev)), json.loads(json.dumps(host)))
    close(json.load(open(tmp_path / "dev" / "curriculum_ablation.json")),
          json.load(open(tmp_path / "host" / "curriculum_ablation.json")))
    assert 0 < CA.BYTES_COPIED["summary"] < records


# ------------------------------------------------------------------ 4. the command line
def test_command_line_prints_the_report(tmp_path, capsys):
    cfg = load_named_config("quick_test")
    cfg.component_ablation.num_episodes, cfg.component_ablation.max_episode_steps = 25, 40
    cfg.output_dir = str(tmp_path / "logs")
    path = tmp_path / "config_short.json"
    cfg.to_json(str(path))
    stats = A.main(["--config", str(path), "--success-rule", "terminated", "--device-streams"])
    out = capsys.readouterr().out
    assert out.startswith("=" * 80 + "\nComponent Ablation Study\n") and "Experiment: quick_test" in out
    assert "  Episodes per run: 25" in out and "  Seeds: [42, 123]" in out
    assert "Component Ablation Report" in out and "Key Insights:" in out
    assert "Warning: Could not generate plots" in out
    assert out.rstrip().endswith("=" * 80) and "Component Ablation Study Complete" in out.split("Key Insights:")[1]
    assert set(stats) == {"baseline", "no_curriculum", "no_dense_reward", "minimal"}
    assert (tmp_path / "logs" / "component_ablation_results.json").exists()
