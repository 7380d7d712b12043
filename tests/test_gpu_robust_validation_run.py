"""GPU: noise-level validation inside PGTrainer.fit (ValidationPlan(noise_levels=...),
dxrl_pg_val_levels_row) on test_gpu_validation_run.py's small trainers (128 envs x 16 steps,
episodes capped at 12 steps), a held-out set of 4 objects x 3 episodes of at most 10 steps, and
the levels (0, 0), (0.05, 0), (0, 0.05), (0.05, 0.05).

Level 0 of a levels plan must be the plan without levels bit for bit (records, main row, best
parameters) and validating must change nothing of the training run; all records must be those of
the same episode program run on a snapshot of the weights; the three tables must be the
restatement's on those records (tests/pg_val_levels_reference.py; bounds as in
test_gpu_pg_val_levels.py); best model, patience and checkpoints must follow the header rules on
the robust score."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pg_val_levels_reference as R
import pg_val_reference as V
import test_gpu_validation_run as TV

pytestmark = pytest.mark.gpu

G, K, VAL_STEPS, VAL_SEED, DEV_SEED = TV.G, TV.K, TV.VAL_STEPS, TV.VAL_SEED, TV.DEV_SEED
LEVELS = [(0.0, 0.0), (0.05, 0.0), (0.0, 0.05), (0.05, 0.05)]
L, GK = len(LEVELS), G * K
# the best-model case: on these two trainers the restatement marks several best rows of
# worst_success_rate in 12 validations of 4 objects x 8 episodes (a2c: rows 0, 2, 4; ppo2x2: 0, 2)
MOVING = [pytest.param(dict(lr=3e-2), id="a2c-lr3e-2"), pytest.param(dict(lr=1e-2, **TV.PPO), id="ppo2x2-lr1e-2")]
MOVING_K = 8


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import envs, evaluation, evaluator, policies, trainer, training_run  # noqa: F401
    return d


def levels_plan(pkg, tr, **kw):
    return TV.plan_of(pkg, tr, noise_levels=kw.pop("noise_levels", LEVELS), **kw)


def level_rows_of(levels_row):
    return [dict(zip(R.LEVEL_COLUMNS, lv)) for lv in np.asarray(levels_row).tolist()]


def check_tables(val, row, rec, iteration, env_steps, train_row):
    """Row `row` of the three tables against the restatement on the records `rec`."""
    rec0 = {k: (v[:GK] if isinstance(v, np.ndarray) else v) for k, v in rec.items()}
    TV.check_row(val.table[row], rec0, iteration, env_steps, train_row)
    main, rows, rob = R.levels_row(LEVELS, G, K, iteration, env_steps, train_row, rec["ep_return"], rec["ep_length"],
                                   rec["ep_success"], rec["ep_contacts"], rec["status"])
    got_levels = val.levels[row]
    for l in range(L):
        got, ref = dict(zip(R.LEVEL_COLUMNS, got_levels[l])), rows[l]
        for name in ("obs_noise_std", "dyn_noise_std", "episodes", "successes", "success_rate", "mean_length",
                     "mean_contacts", "min_object_success_rate", "degradation", "degradation_percentage"):
            assert got[name] == ref[name], (l, name)
        ret = rec["ep_return"][l * GK:(l + 1) * GK]
        bound = TV.sum_bound(ret) / GK
        print("level", l, "mean_return", got["mean_return"], ref["mean_return"], bound, "return_std", got["return_std"],
              ref["return_std"])
        assert abs(got["mean_return"] - ref["mean_return"]) <= bound
        assert abs(got["return_std"] - ref["return_std"]) <= 1e-9 * ref["return_std"]
        assert val.object_successes[row, l].tolist() == \
            V.object_successes(G, K, rec["ep_success"][l * GK:(l + 1) * GK]).tolist()
    dev_rows = R.add_degradation(level_rows_of(got_levels))
    assert R.nan_equal(got_levels, R.level_array(dev_rows))
    assert R.nan_equal(val.robust[row], R.robust_array(R.robust_values(dev_rows)))
    for name in R.ROBUST_COLUMNS[:-1]:  # worst_mean_return is a mean_return: bounded above, not exact
        assert R.nan_equal(val.robust[row, R.RIDX[name]], rob[name]), name
    assert val.level_column("success_rate")[row, 0] == val["success_rate"][row]
    return main, rows, rob


# ------------------------------------------------------------------ (a) level 0 is the plain plan
@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "stochastic"])
@pytest.mark.parametrize("kw", TV.CONFIGS)
def test_level_zero_is_the_plain_plan_and_validating_changes_nothing(pkg, kw, deterministic):
    env_t, twin = TV.make(pkg, **kw)
    log_t = twin.fit(4)
    env_p, plain = TV.make(pkg, **kw)
    plan_p = TV.plan_of(pkg, plain, deterministic=deterministic)
    log_p = plain.fit(4, validation=plan_p, validate_every=2, val_keep_best="mean_return")
    env, tr = TV.make(pkg, **kw)
    plan = levels_plan(pkg, tr, deterministic=deterministic)
    log = tr.fit(4, validation=plan, validate_every=2, val_keep_best="mean_return")
    assert plan.E == L * GK and plan_p.E == GK and "noise_levels" not in plan_p.fingerprint
    assert plan.fingerprint["noise_levels"] == [list(p) for p in LEVELS]
    assert {k: v for k, v in plan.fingerprint.items() if k != "noise_levels"} == plan_p.fingerprint
    for state in (TV.state_of(env_p, plain), TV.state_of(env, tr)):
        TV.assert_same_state(TV.state_of(env_t, twin), state)
    assert log.table.tobytes() == log_p.table.tobytes() == log_t.table.tobytes() and log.header == log_t.header
    assert torch.equal(tr._run.best_params, twin._run.best_params)
    rec, rec_p = TV.records_of(plan), TV.records_of(plan_p)
    assert rec["status"] == rec_p["status"] == 0
    for k in ("ep_return", "ep_length", "ep_success", "ep_contacts"):
        assert rec[k][:GK].tobytes() == rec_p[k].tobytes(), k
    v, vp = log.validation, log_p.validation
    assert len(v) == len(vp) == 2 and v.table.tobytes() == vp.table.tobytes() and v.header == vp.header
    assert v.object_successes[:, 0].tobytes() == vp.object_successes.tobytes()
    assert torch.equal(tr._run.val.best_params, plain._run.val.best_params) and v.best_row is not None
    assert vp.noise_levels is None and vp.levels is None and v.noise_levels == LEVELS
    assert v.levels.shape == (2, L, R.LEVEL_COLS) and v.robust.shape == (2, R.ROBUST_COLS)


# ------------------------------------------------------------------ (b) the records and the tables
@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "stochastic"])
@pytest.mark.parametrize("kw", TV.CONFIGS)
def test_records_are_the_snapshots_and_the_tables_their_restatement(pkg, kw, deterministic):
    from dexterous_rl_manipulation_amd.evaluator import Evaluator, Segment, policy_program
    env, tr = TV.make(pkg, **kw)
    plan = levels_plan(pkg, tr, deterministic=deterministic)
    log = tr.fit(2, validation=plan, validate_every=2, val_keep_best="worst_success_rate")
    rec = TV.records_of(plan)
    assert rec["status"] == 0 and len(rec["ep_return"]) == L * GK
    pol = tr.policy(deterministic=deterministic)
    hs = TV.heldout(pkg)
    ev = Evaluator(pol, hs, max_episode_steps=VAL_STEPS)
    p = ev._program([hs.get_eval_config(i) for i in range(G)])
    for obs, dyn in LEVELS:  # the RobustnessTester's parallel form: one lane per episode, level-major
        for o in range(G):
            for k in range(K):
                p.add_lane([Segment(o, [VAL_SEED + k], obs, dyn, noise_seed=(VAL_SEED, k))])
    snap = p.run(policy_program(pol), host_resets=False, host_noise=False, device_seed=DEV_SEED)
    assert snap.ep_return.tobytes() == rec["ep_return"].tobytes()  # the same kernel, weights and streams
    assert snap.ep_length.tolist() == rec["ep_length"].tolist()
    assert (np.asarray(snap.ep_success) != 0).tolist() == (rec["ep_success"] != 0).tolist()
    assert np.asarray(snap.ep_contacts).tolist() == rec["ep_contacts"].tolist()
    # noise reaches the episodes: some noisy level's records differ from the baseline's
    assert any(rec["ep_return"][l * GK:(l + 1) * GK].tobytes() != rec["ep_return"][:GK].tobytes() for l in range(1, L))
    val = log.validation
    assert len(val) == 1
    main, rows, rob = check_tables(val, 0, rec, 1, 2 * tr.M, 1)
    assert val.header["best_score"] == val.robust_column("worst_success_rate")[0] == rob["worst_success_rate"]
    assert val["is_best"][0] == 1.0 and val.best_iteration == 1
    res = val.level_results(0)
    assert [r["noise_levels"] for r in res] == [{"observation_noise_std": o, "dynamics_noise_std": d} for o, d in LEVELS]
    assert [r["metrics"]["success_rate"] for r in res] == [r["success_rate"] for r in rows]


# ------------------------------------------------------------------ (c) idempotence
def test_two_runs_of_the_plan_give_identical_bytes(pkg):
    env, tr = TV.make(pkg)
    plan = levels_plan(pkg, tr)
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
    assert v.table[0, :V.IS_BEST].tobytes() == v.table[1, :V.IS_BEST].tobytes() == v.table[2, :V.IS_BEST].tobytes()
    assert v.levels[0].tobytes() == v.levels[1].tobytes() == v.levels[2].tobytes()
    assert v.robust[0].tobytes() == v.robust[1].tobytes() == v.robust[2].tobytes()
    assert v.object_successes[0].tobytes() == v.object_successes[1].tobytes() == v.object_successes[2].tobytes()


# ------------------------------------------------------------------ (d) best model on a robust score
@pytest.mark.parametrize("kw", MOVING)
def test_best_policy_under_the_worst_level_is_the_snapshot_of_its_row(pkg, kw):
    env_t, twin = TV.make(pkg, **kw)
    snaps = []
    for _ in range(12):
        twin.iteration()
        torch.cuda.synchronize()
        snaps.append(twin.params.clone())
    env, tr = TV.make(pkg, **kw)
    log = tr.fit(12, validation=levels_plan(pkg, tr, episodes_per_object=MOVING_K), validate_every=1,
                 val_keep_best="worst_success_rate")
    val = log.validation
    score = val.robust_column("worst_success_rate")
    print("worst_success_rate", score.tolist(), "is_best", val["is_best"].tolist(), "clean", val["success_rate"].tolist())
    want_rows, want_header, want_flags = R.robust_series(score.tolist())
    assert len(want_rows) >= 2  # the case was picked so that the restatement alone improves more than once
    assert val["is_best"].tolist() == want_flags[:, 0].tolist() and val["since_best"].tolist() == want_flags[:, 1].tolist()
    assert val.header == want_header
    b = val.best_row
    assert b == want_rows[-1] == int(np.argmax(score)) and 0 < b < 11 and val.best_iteration == b
    assert val.header["best_score"] == score[b] == val.level_column("success_rate")[b].min()
    assert val.robust_column("worst_level")[b] == int(np.argmin(val.level_column("success_rate")[b]))
    assert torch.equal(tr._run.val.best_params, snaps[b])  # bit for bit
    got, want = tr.best_policy(which="validation"), pkg.policies.MLPActorPolicy.from_params(snaps[b])
    for name in ("W1a", "W2a", "W3a", "logstd"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    clean_rows = V.series_rules(val["success_rate"].tolist(), score_name="success_rate")[0]
    print("best rows by the clean success_rate", clean_rows, "by worst_success_rate", want_rows)


# ------------------------------------------------------------------ (e) patience on a robust score
def test_patience_on_the_robust_score_stops_where_the_restatement_predicts(pkg):
    kw = dict(lr=3e-2)
    settings = dict(validate_every=1, val_keep_best="worst_success_rate", patience=2)
    env_f, full = TV.make(pkg, **kw)
    log_f = full.fit(12, validation=levels_plan(pkg, full, episodes_per_object=MOVING_K), **settings)
    curve = log_f.validation.robust_column("worst_success_rate").tolist()
    _, want, _ = R.robust_series(curve, patience=2)
    print("curve", curve, "stopped_row", want["stopped_row"])
    assert len(log_f) == 12 and log_f.validation.header == want
    s = want["stopped_row"]
    assert 2 <= s < 11  # after a later best row, before the run's end
    env, tr = TV.make(pkg, **kw)
    log = tr.fit(12, validation=levels_plan(pkg, tr, episodes_per_object=MOVING_K), poll_every=1,
                 stop_on_patience=True, **settings)
    assert len(log) == s + 1 and tr.iteration_index == s + 1 and tr._run.host_reads == s + 1
    v = log.validation
    assert v.stopped_iteration == s and len(v) == s + 1
    assert v.table.tobytes() == log_f.validation.table[:s + 1].tobytes()
    assert v.levels.tobytes() == log_f.validation.levels[:s + 1].tobytes()
    assert v.robust.tobytes() == log_f.validation.robust[:s + 1].tobytes()


# ------------------------------------------------------------------ (f) no host reads
def test_fit_with_levels_and_no_polling_reads_nothing(pkg):
    env, tr = TV.make(pkg, **TV.PPO)
    plan = levels_plan(pkg, tr, deterministic=False)
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
    assert log.validation.levels.shape == (3, L, R.LEVEL_COLS)


# ------------------------------------------------------------------ (g) checkpoints
def test_resume_continues_all_three_tables_bit_for_bit(pkg, tmp_path):
    settings = dict(validate_every=1, val_keep_best="mean_success_rate", patience=2)
    env_b, b = TV.make(pkg, **TV.PPO)
    log_b = b.fit(4, validation=levels_plan(pkg, b), **settings)
    env_a, a = TV.make(pkg, **TV.PPO)
    a.fit(2, validation=levels_plan(pkg, a), **settings)
    path = tmp_path / "ck.npz"
    a.save_checkpoint(path)
    r = pkg.trainer.PGTrainer.load_checkpoint(path, TV.make_env(pkg))
    assert r._run.val is not None and r._run.val.rows == 2 and r._run.val.L == L
    with pytest.raises(ValueError, match="noise_levels"):
        r.fit(1, validation=levels_plan(pkg, r, noise_levels=LEVELS[:3]), **settings)
    with pytest.raises(ValueError, match="noise_levels"):
        r.fit(1, validation=TV.plan_of(pkg, r), **settings)  # a plan without levels is another plan too
    assert r.iteration_index == 2  # a refused plan ran nothing
    log_r = r.fit(2, validation=levels_plan(pkg, r), **settings)
    TV.assert_same_state(TV.state_of(env_b, b), TV.state_of(r.env, r))
    assert log_r.table.tobytes() == log_b.table.tobytes() and log_r.header == log_b.header
    vr, vb = log_r.validation, log_b.validation
    assert len(vr) == 4 and vr.table.tobytes() == vb.table.tobytes() and vr.header == vb.header
    assert vr.levels.tobytes() == vb.levels.tobytes() and vr.robust.tobytes() == vb.robust.tobytes()
    assert vr.object_successes.tobytes() == vb.object_successes.tobytes() and vr.noise_levels == vb.noise_levels
    assert torch.equal(r._run.val.best_params, b._run.val.best_params)
    arrays, meta = pkg.training_run.read_checkpoint(path)
    assert arrays["val_levels"].shape == (2, L, R.LEVEL_COLS) and arrays["val_robust"].shape == (2, R.ROBUST_COLS)
    assert arrays["val_objects"].shape == (2, L, G)
    ck = pkg.training_run.validation_log_of_checkpoint(arrays, meta)
    assert ck.levels.tobytes() == vb.levels[:2].tobytes() and ck.noise_levels == LEVELS


def test_a_checkpoint_written_before_levels_existed_still_loads(pkg, tmp_path):
    env_a, a = TV.make(pkg)
    a.fit(2, validation=TV.plan_of(pkg, a), validate_every=1)
    new = tmp_path / "new.npz"
    a.save_checkpoint(new)
    arrays, meta = pkg.training_run.read_checkpoint(new)
    # a plan without levels writes what the parent commit wrote: no optional level entries at all
    assert not {"val_levels", "val_robust"} & set(arrays) and "noise_levels" not in meta["validation"]["fingerprint"]
    old = tmp_path / "old.npz"
    pkg.training_run.write_checkpoint(old, {k: v for k, v in arrays.items() if k not in ("val_levels", "val_robust")},
                                      {k: v for k, v in meta.items() if k != "format"})
    r = pkg.trainer.PGTrainer.load_checkpoint(old, TV.make_env(pkg))
    assert r._run.val.rows == 2 and r._run.val.L == 0 and r._run.val.levels is None
    log = r.fit(1, validation=TV.plan_of(pkg, r), validate_every=1)
    assert len(log.validation) == 3 and log.validation.levels is None
    with pytest.raises(ValueError, match="noise_levels"):
        r.fit(1, validation=levels_plan(pkg, r))


# ------------------------------------------------------------------ (h) the CLI, in a child process
def test_cli_child_process_writes_the_levels_and_the_best_policy(pkg, tmp_path):
    from dexterous_rl_manipulation_amd import training_run
    args = ["--config-name", "easy", "--envs", "128", "--horizon", "16", "--max-steps", "12", "--iterations", "3",
            "--validate-every", "1", "--val-episodes", "2", "--val-seed", "7", "--val-obs-noise", "0.05",
            "--val-dyn-noise", "0.05", "--val-keep-best", "worst_success_rate"]
    child = tmp_path / "child"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([TV.ROOT] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-m", "dexterous_rl_manipulation_amd.train"] + args + ["--out", str(child)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("training_log.json", "checkpoint.npz", "best_val_policy.npz"):
        assert (child / name).exists(), name
    v = training_run.TrainingLog.load(child / "training_log.json").validation
    assert v.noise_levels == LEVELS and len(v) == 3 and v["episodes"].tolist() == [40.0] * 3
    assert v.levels.shape == (3, L, R.LEVEL_COLS) and v.robust.shape == (3, R.ROBUST_COLS)
    assert v.object_successes.shape == (3, L, 20) and v.settings["val_keep_best"] == "worst_success_rate"
    assert v.level_column("episodes").tolist() == [[40.0] * L] * 3
    assert v.best_row is not None and v.header["best_score"] == v.robust_column("worst_success_rate")[v.best_row]
    dev_rows = R.add_degradation(level_rows_of(v.levels[2]))
    assert R.nan_equal(v.robust[2], R.robust_array(R.robust_values(dev_rows)))
    pol = pkg.policies.MLPActorPolicy.load(child / "best_val_policy.npz")
    assert pol.W1a.shape == (256, 64)
    arrays, meta = training_run.read_checkpoint(child / "checkpoint.npz")
    assert meta["validation"]["rows"] == 3 and arrays["val_levels"].shape == (3, L, R.LEVEL_COLS)


# ------------------------------------------------------------------ (i) what raises
def test_robust_scores_need_levels_and_bad_plans_and_collective_trainers_raise(pkg):
    env, tr = TV.make(pkg)
    for name in R.ROBUST_SCORES:
        with pytest.raises(ValueError, match="noise_levels"):
            tr.fit(1, validation=TV.plan_of(pkg, tr), val_keep_best=name)
        with pytest.raises(ValueError, match="noise_levels"):
            tr.fit(1, val_keep_best=name)  # no plan at all
    with pytest.raises(ValueError):
        tr.fit(1, validation=levels_plan(pkg, tr), val_keep_best="worst_level")
    for bad in ([(0.1, 0.0), (0.1, 0.0)], [(-0.1, 0.0)], [(float("nan"), 0.0)],
                [(0.01 * k, 0.0) for k in range(1, 17)]):
        with pytest.raises(ValueError):
            levels_plan(pkg, tr, noise_levels=bad)
    with pytest.raises(ValueError, match="256"):
        tr.validation_plan(TV.heldout(pkg, objects=257), episodes_per_object=1, noise_levels=LEVELS)
    assert levels_plan(pkg, tr, noise_levels=[(0.05, 0.0)]).noise_levels == [(0.0, 0.0), (0.05, 0.0)]
    assert tr.iteration_index == 0
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        col = pkg.trainer.PGTrainer(TV.make_env(pkg), pkg.trainer.TrainerConfig(horizon=16, seed=1),
                                    process_group=dist.group.WORLD, world_size=1)
        with pytest.raises(ValueError, match="one rank"):
            col.fit(1, validation=levels_plan(pkg, tr), val_keep_best="worst_success_rate")
        assert col.iteration_index == 0
    finally:
        dist.destroy_process_group()
