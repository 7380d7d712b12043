"""GPU: common random numbers across the noise levels of a validation inside PGTrainer.fit
(ValidationPlan(noise_levels=..., common_random_numbers=True), dxrl_evaluate_mlp with
stream_period = G K, dxrl_pg_val_paired_row) on test_gpu_validation_run.py's small trainers and
held-out set with test_gpu_robust_validation_run.py's levels.

The option must leave the baseline alone (level 0's records, the main row, the best parameters of
a main-row score and the training state are the plain plan's and the non-CRN levels plan's bit
for bit); the records must be the snapshot program's with stream_period = G K; the levels and
robust tables the existing restatement on those records and the paired table the new one
(tests/pg_val_paired_reference.py; bounds as in test_gpu_pg_val_paired.py); and the five tables
must repeat, resume and travel through the checkpoint and the CLI."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pg_val_paired_reference as P
import test_gpu_robust_validation_run as TR
import test_gpu_validation_run as TV

pytestmark = pytest.mark.gpu

G, K, VAL_STEPS, VAL_SEED, DEV_SEED = TV.G, TV.K, TV.VAL_STEPS, TV.VAL_SEED, TV.DEV_SEED
LEVELS, L, GK = TR.LEVELS, TR.L, TR.GK


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import envs, evaluation, evaluator, policies, trainer, training_run  # noqa: F401
    return d


def crn_plan(pkg, tr, **kw):
    return TR.levels_plan(pkg, tr, common_random_numbers=True, **kw)


def check_paired(val, row, rec):
    """Row `row` of the paired table and of object_lost against the restatement on the records."""
    rows, lost = P.paired_row(L, G, K, rec["ep_return"], rec["ep_length"], rec["ep_success"])
    assert val.object_lost[row].tolist() == lost.tolist()
    for l in range(L):
        got, ref = dict(zip(P.PAIRED_COLUMNS, val.paired[row, l])), rows[l]
        for name in P.INTEGER_COLUMNS + ("mean_length_diff",):
            assert got[name] == ref[name], (l, name)
        dev = P.derived(got["lost"], got["gained"], got["pairs"])
        for name in P.DERIVED_COLUMNS:
            assert got[name] == dev[name] == ref[name], (l, name)
        ret0, ret1 = rec["ep_return"][:GK], rec["ep_return"][l * GK:(l + 1) * GK]
        mean, std, stderr = P.two_pass(ret0, ret1)
        bound = P.sum_bound(ret1 - ret0) / GK
        print("level", l, "mean_return_diff", got["mean_return_diff"], mean, bound, "std", got["return_diff_std"], std)
        assert abs(got["mean_return_diff"] - mean) <= bound
        for have, want in ((got["return_diff_std"], std), (got["return_diff_stderr"], stderr)):
            assert have == 0.0 if want == 0.0 else abs(have - want) <= 1e-9 * want
        # consistency with the level table: exactly
        successes = val.level_column("successes")[row]
        assert got["lost"] - got["gained"] == successes[0] - successes[l]
    assert np.all(val.paired[row, 0, P.PIDX["mean_return_diff"]:] == 0.0)  # the baseline against itself
    return rows


# ------------------------------------------------------------------ (a) the baseline is unchanged
@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "stochastic"])
@pytest.mark.parametrize("kw", TV.CONFIGS)
def test_the_baseline_and_the_training_run_are_unchanged(pkg, kw, deterministic):
    settings = dict(validate_every=2, val_keep_best="mean_return")
    env_p, plain = TV.make(pkg, **kw)
    plan_p = TV.plan_of(pkg, plain, deterministic=deterministic)
    log_p = plain.fit(4, validation=plan_p, **settings)
    env_l, lev = TV.make(pkg, **kw)
    plan_l = TR.levels_plan(pkg, lev, deterministic=deterministic)
    log_l = lev.fit(4, validation=plan_l, **settings)
    env, tr = TV.make(pkg, **kw)
    plan = crn_plan(pkg, tr, deterministic=deterministic)
    log = tr.fit(4, validation=plan, **settings)
    assert plan.fingerprint == dict(plan_l.fingerprint, common_random_numbers=True)
    assert "common_random_numbers" not in plan_l.fingerprint and "common_random_numbers" not in plan_p.fingerprint
    assert plan.args.stream_period == GK and plan_l.args.stream_period == plan_p.args.stream_period == 0
    for other_env, other in ((env_p, plain), (env_l, lev)):
        TV.assert_same_state(TV.state_of(other_env, other), TV.state_of(env, tr))
        assert torch.equal(tr._run.best_params, other._run.best_params)
        assert torch.equal(tr._run.val.best_params, other._run.val.best_params)
    assert log.table.tobytes() == log_p.table.tobytes() == log_l.table.tobytes() and log.header == log_p.header
    rec, rec_p, rec_l = TV.records_of(plan), TV.records_of(plan_p), TV.records_of(plan_l)
    assert rec["status"] == 0
    for k in ("ep_return", "ep_length", "ep_success", "ep_contacts"):
        assert rec[k][:GK].tobytes() == rec_p[k].tobytes() == rec_l[k][:GK].tobytes(), k
    assert rec["ep_return"][GK:].tobytes() != rec_l["ep_return"][GK:].tobytes()  # the noisy levels are other episodes
    v, vp, vl = log.validation, log_p.validation, log_l.validation
    assert len(v) == 2 and v.best_row is not None
    assert v.table.tobytes() == vp.table.tobytes() == vl.table.tobytes() and v.header == vp.header == vl.header
    assert v.levels[:, 0].tobytes() == vl.levels[:, 0].tobytes()
    assert v.object_successes[:, 0].tobytes() == vp.object_successes.tobytes()
    assert vl.paired is None and vl.object_lost is None and vp.paired is None
    assert v.paired.shape == (2, L, P.PAIRED_COLS) and v.object_lost.shape == (2, L, G)


# ------------------------------------------------------------------ (b) the records and the tables
@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "stochastic"])
@pytest.mark.parametrize("kw", TV.CONFIGS)
def test_records_are_the_snapshots_and_the_tables_their_restatement(pkg, kw, deterministic):
    from dexterous_rl_manipulation_amd.evaluator import Evaluator, Segment, policy_program
    env, tr = TV.make(pkg, **kw)
    plan = crn_plan(pkg, tr, deterministic=deterministic)
    log = tr.fit(2, validation=plan, validate_every=2, val_keep_best="worst_success_rate")
    rec = TV.records_of(plan)
    assert rec["status"] == 0 and len(rec["ep_return"]) == L * GK
    pol = tr.policy(deterministic=deterministic)
    hs = TV.heldout(pkg)
    ev = Evaluator(pol, hs, max_episode_steps=VAL_STEPS)
    p = ev._program([hs.get_eval_config(i) for i in range(G)])
    for obs, dyn in LEVELS:
        for o in range(G):
            for k in range(K):
                p.add_lane([Segment(o, [VAL_SEED + k], obs, dyn, noise_seed=(VAL_SEED, k))])
    snap = p.run(policy_program(pol), host_resets=False, host_noise=False, device_seed=DEV_SEED, stream_period=GK)
    assert snap.ep_return.tobytes() == rec["ep_return"].tobytes()  # the same kernel, weights and streams
    assert snap.ep_length.tolist() == rec["ep_length"].tolist()
    assert (np.asarray(snap.ep_success) != 0).tolist() == (rec["ep_success"] != 0).tolist()
    assert np.asarray(snap.ep_contacts).tolist() == rec["ep_contacts"].tolist()
    plain = p.run(policy_program(pol), host_resets=False, host_noise=False, device_seed=DEV_SEED)
    assert plain.ep_return[:GK].tobytes() == snap.ep_return[:GK].tobytes()
    assert plain.ep_return[GK:].tobytes() != snap.ep_return[GK:].tobytes()
    val = log.validation
    assert len(val) == 1
    main, rows, rob = TR.check_tables(val, 0, rec, 1, 2 * tr.M, 1)
    assert val.header["best_score"] == val.robust_column("worst_success_rate")[0] == rob["worst_success_rate"]
    check_paired(val, 0, rec)
    st = val.statistics()
    assert st["common_random_numbers"] is True and st["final_max_lost"] == val.paired_column("lost")[0, 1:].max()
    assert st["final_min_mean_return_diff"] == val.paired_column("mean_return_diff")[0, 1:].min()


# ------------------------------------------------------------------ (c) repeatability
def test_two_runs_of_the_plan_give_identical_bytes(pkg):
    env, tr = TV.make(pkg)
    plan = crn_plan(pkg, tr)
    tr.fit(1, validation=plan)
    first = TV.records_of(plan)
    val = tr._run.val
    for _ in range(2):
        plan.run(tr, val, 0, tr.M, 0)
    again = TV.records_of(plan)
    for k in first:
        assert np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes(), k
    v = tr.training_log().validation
    assert len(v) == 3
    for t in (v.levels, v.robust, v.object_successes, v.paired, v.object_lost):
        assert t[0].tobytes() == t[1].tobytes() == t[2].tobytes()
    check_paired(v, 2, again)


# ------------------------------------------------------------------ (d) checkpoints
def test_resume_continues_all_five_tables_bit_for_bit(pkg, tmp_path):
    settings = dict(validate_every=1, val_keep_best="mean_success_rate", patience=2)
    env_b, b = TV.make(pkg, **TV.PPO)
    log_b = b.fit(4, validation=crn_plan(pkg, b), **settings)
    env_a, a = TV.make(pkg, **TV.PPO)
    a.fit(2, validation=crn_plan(pkg, a), **settings)
    path = tmp_path / "ck.npz"
    a.save_checkpoint(path)
    r = pkg.trainer.PGTrainer.load_checkpoint(path, TV.make_env(pkg))
    assert r._run.val is not None and r._run.val.rows == 2 and r._run.val.L == L and r._run.val.crn
    with pytest.raises(ValueError, match="common_random_numbers"):
        r.fit(1, validation=TR.levels_plan(pkg, r), **settings)  # the other setting is another plan
    assert r.iteration_index == 2  # a refused plan ran nothing
    log_r = r.fit(2, validation=crn_plan(pkg, r), **settings)
    TV.assert_same_state(TV.state_of(env_b, b), TV.state_of(r.env, r))
    assert log_r.table.tobytes() == log_b.table.tobytes() and log_r.header == log_b.header
    vr, vb = log_r.validation, log_b.validation
    assert len(vr) == 4 and vr.table.tobytes() == vb.table.tobytes() and vr.header == vb.header
    assert vr.levels.tobytes() == vb.levels.tobytes() and vr.robust.tobytes() == vb.robust.tobytes()
    assert vr.object_successes.tobytes() == vb.object_successes.tobytes()
    assert vr.paired.tobytes() == vb.paired.tobytes() and vr.object_lost.tobytes() == vb.object_lost.tobytes()
    assert torch.equal(r._run.val.best_params, b._run.val.best_params)
    arrays, meta = pkg.training_run.read_checkpoint(path)
    assert arrays["val_paired"].shape == (2, L, P.PAIRED_COLS) and arrays["val_object_lost"].shape == (2, L, G)
    assert meta["validation"]["fingerprint"]["common_random_numbers"] is True
    ck = pkg.training_run.validation_log_of_checkpoint(arrays, meta)
    assert ck.paired.tobytes() == vb.paired[:2].tobytes() and ck.object_lost.tobytes() == vb.object_lost[:2].tobytes()


def test_a_checkpoint_without_the_entries_loads_and_the_other_setting_raises(pkg, tmp_path):
    env_a, a = TV.make(pkg)
    a.fit(2, validation=TR.levels_plan(pkg, a), validate_every=1)
    path = tmp_path / "levels.npz"
    a.save_checkpoint(path)
    arrays, meta = pkg.training_run.read_checkpoint(path)
    # a plan without the option writes what the parent commit wrote: no paired entries, no key
    assert not {"val_paired", "val_object_lost"} & set(arrays)
    assert "common_random_numbers" not in meta["validation"]["fingerprint"]
    r = pkg.trainer.PGTrainer.load_checkpoint(path, TV.make_env(pkg))
    assert r._run.val.rows == 2 and not r._run.val.crn and r._run.val.paired is None
    with pytest.raises(ValueError, match="common_random_numbers"):
        r.fit(1, validation=crn_plan(pkg, r), validate_every=1)
    log = r.fit(1, validation=TR.levels_plan(pkg, r), validate_every=1)
    assert len(log.validation) == 3 and log.validation.paired is None
    with pytest.raises(ValueError, match="noise_levels"):
        TV.plan_of(pkg, r, common_random_numbers=True)  # the option needs levels


# ------------------------------------------------------------------ (e) the CLI, in a child process
def test_cli_child_process_writes_the_paired_table(pkg, tmp_path):
    from dexterous_rl_manipulation_amd import training_run
    args = ["--config-name", "easy", "--envs", "128", "--horizon", "16", "--max-steps", "12", "--iterations", "2",
            "--validate-every", "1", "--val-episodes", "2", "--val-seed", "7", "--val-obs-noise", "0.05",
            "--val-dyn-noise", "0.05", "--val-keep-best", "worst_success_rate", "--val-common-random-numbers"]
    child = tmp_path / "child"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([TV.ROOT] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-m", "dexterous_rl_manipulation_amd.train"] + args + ["--out", str(child)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    v = training_run.TrainingLog.load(child / "training_log.json").validation
    assert v.noise_levels == LEVELS and len(v) == 2
    assert v.paired.shape == (2, L, P.PAIRED_COLS) and v.object_lost.shape == (2, L, 20)
    assert v.paired_column("pairs").tolist() == [[40.0] * L] * 2
    successes = v.level_column("successes")
    assert np.array_equal(v.paired_column("lost") - v.paired_column("gained"), successes[:, :1] - successes)
    assert np.array_equal(v.object_lost.sum(axis=2), v.paired_column("lost"))
    assert not math.isnan(v.paired_column("return_diff_stderr")[-1, -1])
    arrays, meta = training_run.read_checkpoint(child / "checkpoint.npz")
    assert arrays["val_paired"].shape == (2, L, P.PAIRED_COLS)
    assert meta["validation"]["fingerprint"]["common_random_numbers"] is True


# ------------------------------------------------------------------ (f) no host reads
def test_fit_with_common_random_numbers_and_no_polling_reads_nothing(pkg):
    env, tr = TV.make(pkg, **TV.PPO)
    plan = crn_plan(pkg, tr, deterministic=False)
    print("set_sync_debug_mode('error') enforced by this build:", TV.sync_debug_mode_works())
    torch.cuda.set_sync_debug_mode("error")
    try:
        log = tr.fit(3, poll_every=0, validation=plan, validate_every=1, val_keep_best="mean_noisy_success_rate",
                     patience=1, stop_on_patience=True)
        reads = tr._run.host_reads
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reads == 0
    assert len(log) == 3 and log.validation["iteration"].tolist() == [0.0, 1.0, 2.0]
    assert log.validation.paired.shape == (3, L, P.PAIRED_COLS)
