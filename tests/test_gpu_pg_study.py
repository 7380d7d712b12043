"""GPU: the component ablation of the policy-gradient trainer (training_study.run_training_study,
ablation.run_pg_component_study, the pg_ablation command) on the small trainers of
test_gpu_validation_run.py: 128 envs x 16 steps, episodes capped at 12 steps, a held-out set of
4 objects x 3 episodes of at most 10 steps; 4 arms x 2 seeds x 6 iterations, validated every 2,
W = 2.

The study must change nothing of a run (every run's rows in the two slabs are the bytes of a
stand-alone fit of the same job), its run table must agree with every run's own log header, and
the device summary with the NumPy one within the bounds of tests/test_gpu_pg_runs.py."""
import json

import numpy as np
import pytest
import torch

import pg_runs_reference as P

pytestmark = pytest.mark.gpu

SEEDS, ITERATIONS, EVERY, W, THR = (42, 123), 6, 2, 2, 0.05
JOB = dict(num_envs=128, horizon=16, max_steps=12, validate_every=EVERY, val_episodes=3, val_seed=5, val_max_steps=10,
           ent_coef=0.01)


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import ablation, evaluation, training_study  # noqa: F401
    return d


def heldout(pkg):
    return pkg.evaluation.HeldOutObjectSet(pkg.CurriculumConfig.variable(), num_heldout_objects=4, seed=42)


def specs(pkg):
    from dexterous_rl_manipulation_amd import ablation
    return ablation.pg_study_specs(window=W, threshold=THR, final_window=W)


@pytest.fixture(scope="module")
def study(pkg):
    from dexterous_rl_manipulation_amd import ablation
    stats, result = ablation.run_pg_component_study(ITERATIONS, SEEDS, convergence_window=W, convergence_threshold=THR,
                                                    final_window=W, return_study=True, return_logs=True,
                                                    heldout_set=heldout(pkg), **JOB)
    torch.cuda.synchronize()
    return stats, result, {name: result.tables(name) for name in ("training", "validation")}


def test_every_run_is_the_stand_alone_fit_and_the_run_table_its_header(pkg, study):
    from dexterous_rl_manipulation_amd import ablation, training_study as T
    _, result, tables = study
    assert result.run_rows["training"] == [ITERATIONS] * 8 and result.run_rows["validation"] == [ITERATIONS // EVERY] * 8
    assert tables["training"].shape == (8, ITERATIONS, 24) and tables["validation"].shape[2] == 16
    easy, hard = pkg.CurriculumConfig.easy().to_state(), pkg.CurriculumConfig.hard().to_state()
    train, val = result.training, result.validation
    for arm in ablation.pg_component_arms():
        for seed in SEEDS:
            r = result.run_index(arm.name, seed)
            env, tr, fit_kw = T.make_job(arm, seed, heldout_set=heldout(pkg), train_spec=specs(pkg)[0], **JOB)
            # a curriculum arm starts on the scheduler's easy config, the others train on the hard one
            assert env.curriculum_configs[0].to_state() == (easy if arm.use_curriculum else hard)
            assert env.reward_type == arm.reward_type
            log = tr.fit(ITERATIONS, **fit_kw)
            assert tables["training"][r].tobytes() == log.table.tobytes(), (arm.name, seed)
            assert tables["validation"][r, :len(log.validation)].tobytes() == log.validation.table.tobytes()
            assert result.logs[r].table.tobytes() == log.table.tobytes()
            # the spec fit was given: the device header's rows are the run table's
            conv = -1 if log.converged_row is None else log.converged_row
            best = -1 if log.best_row is None else log.best_row
            assert train.run("success_rate", "convergence_row")[r] == conv
            assert train.run("success_rate", "best_row")[r] == best
            if best >= 0:
                assert train.run("success_rate", "best")[r] == log.header["best_score"]
            # the validation keep-best follows the same rule on the held-out success rate
            vbest = -1 if log.validation.best_row is None else log.validation.best_row
            assert val.run("success_rate", "best_row")[r] == vbest
            assert tr._run.host_reads == 0
            assert result.progression_steps[r] == (len(tr.scheduler.progression_history) if arm.use_curriculum
                                                   else None)
            T.release_job(env, tr, fit_kw)
    assert result.host_reads == [0] * 8
    assert result.status() == {"training": 0, "validation": 0}


def test_arms_differ_where_they_should(pkg, study):
    _, result, tables = study
    from dexterous_rl_manipulation_amd import _native as N
    ret = N.PG_LOG_COLUMNS.index("mean_step_reward")
    for seed in SEEDS:
        dense, sparse = result.run_index("baseline", seed), result.run_index("no_dense_reward", seed)
        assert not np.array_equal(tables["training"][dense], tables["training"][sparse], equal_nan=True)
        assert not np.array_equal(tables["training"][dense, :, ret], tables["training"][sparse, :, ret])
        cur, fixed = result.run_index("baseline", seed), result.run_index("no_curriculum", seed)
        assert not np.array_equal(tables["training"][cur], tables["training"][fixed], equal_nan=True)
    a, b = result.run_index("baseline", SEEDS[0]), result.run_index("baseline", SEEDS[1])
    assert not np.array_equal(tables["training"][a], tables["training"][b], equal_nan=True)
    # the same held-out plan in every job: the same iterations and env steps in every validation table
    it = N.PG_VAL_COLUMNS.index("iteration")
    assert (tables["validation"][:, :3, it] == [1.0, 3.0, 5.0]).all()
    assert (tables["validation"][:, :3, N.PG_VAL_COLUMNS.index("episodes")] == 12.0).all()
    assert (tables["validation"][:, 3:] == 0.0).all()  # the slab's spare row stays as allocated


def test_device_and_host_summaries_agree(pkg, study):
    from dexterous_rl_manipulation_amd import ablation, training_study as T
    _, result, tables = study
    arms = result.arms
    off, flat = T.csr_groups([[a * len(SEEDS) + k for k in range(len(SEEDS))] for a in range(len(arms))])
    weights = T.contrast_matrix(arms, ablation.PG_COMPONENT_CONTRASTS)
    for name in ("training", "validation"):
        slab = result.slab(name)
        nat = T.native_specs(slab.specs, name)
        tuples = [(s.col, s.x_col, s.window, s.threshold, s.final_window) for s in nat]
        got = (slab.run_table, slab.group_table, slab.contrast_table, slab.status)
        host = T.summarize_host(tables[name], result.run_rows[name], nat, off, flat, weights)
        P.check_tables(got, host, tables[name], result.run_rows[name], tuples, off, flat, weights)
        want = P.summarize(tables[name], result.run_rows[name], tuples, off, flat, weights)
        P.check_tables(got, want, tables[name], result.run_rows[name], tuples, off, flat, weights)
    # the device summary copies the three small tables, the host path the slabs
    sizes = [t.size * 8 + 4 for s in (result.training, result.validation)
             for t in [np.concatenate([s.run_table.ravel(), s.group_table.ravel(), s.contrast_table.ravel()])]]
    assert result.bytes_copied == sum(sizes) and result.device_summary


def test_host_summary_flag_gives_the_same_tables(pkg):
    """device_summary=False on a small study (2 arms x 2 seeds x 3 iterations) against the device
    summary of the slabs that study filled."""
    from dexterous_rl_manipulation_amd import ablation, training_study as T
    arms = ablation.pg_component_arms()[:2]
    contrasts = {"no_curriculum_vs_baseline": ablation.PG_COMPONENT_CONTRASTS["no_curriculum_vs_baseline"]}
    result = T.run_training_study(arms, SEEDS, 3, heldout_set=heldout(pkg), train_specs=specs(pkg),
                                  val_specs=specs(pkg), contrasts=contrasts, device_summary=False, **JOB)
    assert not result.device_summary and result.logs is None and result.host_reads == [0] * 4
    off, flat = T.csr_groups([[0, 1], [2, 3]])
    weights = T.contrast_matrix(result.arms, contrasts)
    copied = 0
    for name in ("training", "validation"):
        slab = result.slab(name)
        nat = T.native_specs(slab.specs, name)
        pending, _ = T.summarize_device(result.slabs[name], result.run_rows[name], nat, off, flat, weights)
        dev = T.SlabSummary(name, slab.specs, result.run_names, result.arms, list(contrasts), _pending=pending)
        tuples = [(s.col, s.x_col, s.window, s.threshold, s.final_window) for s in nat]
        tables = result.tables(name)
        copied += tables.nbytes
        P.check_tables((dev.run_table, dev.group_table, dev.contrast_table, dev.status),
                       (slab.run_table, slab.group_table, slab.contrast_table, slab.status), tables,
                       result.run_rows[name], tuples, off, flat, weights)
    assert result.bytes_copied == copied
    assert result.run_rows["validation"] == [2] * 4  # after iteration 2 and after the last one


def test_statistics_dictionary_and_report(pkg, study, capsys):
    from dexterous_rl_manipulation_amd import ablation
    stats, result, tables = study
    assert list(stats) == [a for a, _, _ in ablation.ABLATION_CONFIGS] + ["effects"]
    val = result.validation
    sr = 5  # success_rate in the validation table
    for a, arm in enumerate(result.arms):
        rows = ITERATIONS // EVERY
        finals = [tables["validation"][a * 2 + k, rows - W:rows, sr] for k in range(2)]
        want = np.mean([(f[0] + f[1]) / W for f in finals])
        assert stats[arm]["final_success_rate"]["mean"] == pytest.approx(want, rel=1e-12, abs=1e-15)
        assert stats[arm]["final_success_rate"]["min"] == min((f[0] + f[1]) / W for f in finals)
        n = stats[arm]["convergence_step"]["num_converged"]
        assert n == int((val.run("success_rate", "convergence_row")[a * 2:a * 2 + 2] >= 0).sum())
        assert (stats[arm]["convergence_step"]["mean"] is None) == (n == 0)
    assert set(stats["effects"]) == set(ablation.PG_COMPONENT_CONTRASTS)
    for e in stats["effects"].values():
        assert e["pairs"] == len(SEEDS) and np.isfinite(e["mean"]) and e["stderr"] >= 0.0
    ablation.print_ablation_report({}, stats)
    out = capsys.readouterr().out
    assert "Component Ablation Report" in out and "Baseline (Curriculum + Dense Reward):" in out
    assert "No Dense Reward:" in out and "3. Combined Impact:" in out
    json.dumps(result.to_dict(), allow_nan=False)


def test_command_writes_its_json(pkg, tmp_path, capsys):
    from dexterous_rl_manipulation_amd import ablation, pg_ablation
    assert pg_ablation.main(["--iterations", "3", "--envs", "128", "--horizon", "16", "--seeds", "42", "123",
                             "--out", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    assert "Component Ablation Report" in out and "Paired effects on the final success rate" in out
    d = json.loads((tmp_path / pg_ablation.JSON_NAME).read_text())
    assert set(d) == {"statistics", "study"}
    assert list(d["statistics"]) == [a for a, _, _ in ablation.ABLATION_CONFIGS] + ["effects"]
    s = d["study"]
    assert s["arms"] == [a for a, _, _ in ablation.ABLATION_CONFIGS] and s["seeds"] == [42, 123]
    assert s["iterations"] == 3 and s["host_reads"] == [0] * 8 and s["device_summary"] is True
    assert np.array(s["training"]["run_table"], dtype=object).shape == (8, 3, 8)
    assert [row[0][0] for row in s["training"]["run_table"]] == [3.0] * 8       # rows per run
    assert [row[0][0] for row in s["validation"]["run_table"]] == [1.0] * 8     # validated after the last iteration
    assert s["settings"]["max_steps"] == 200 and s["settings"]["val_episodes"] == 5
