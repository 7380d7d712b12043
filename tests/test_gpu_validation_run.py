"""GPU: held-out validation inside PGTrainer.fit (training_run.ValidationPlan, dxrl_pg_val_row)
on small trainers (128 envs x 16 steps, episodes capped at 12 steps, as test_gpu_training_run.py)
with a held-out set of 4 objects x 3 episodes of at most 10 steps.

Validation must change nothing of the training run, its episode records must be the Evaluator's
on a snapshot of the same weights (same kernel, same streams: bit for bit), its row the
restatement's on those records (tests/pg_val_reference.py; integers exact, the mean within
k 2^-52 sum|x| / k, the standard deviation within 1e-9 relative), and best model, patience and
checkpoints must follow the header rules."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pg_val_reference as V

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
PPO = dict(epochs=2, minibatches=2)
CONFIGS = [pytest.param({}, id="a2c"), pytest.param(PPO, id="ppo2x2")]
G, K, VAL_STEPS, VAL_SEED, DEV_SEED = 4, 3, 10, 5, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import envs, evaluation, evaluator, trainer, training_run  # noqa: F401
    return d


def make_env(pkg, n=128):
    return pkg.envs.VecEnv(n, curriculum_config=pkg.CurriculumConfig.variable(), reward_type="dense", seed=3)


def make(pkg, n=128, T=16, **kw):
    env = make_env(pkg, n)
    tr = pkg.trainer.PGTrainer(env, pkg.trainer.TrainerConfig(horizon=T, seed=1, ent_coef=0.01, max_steps=12, **kw))
    env.reset(write_obs=False)
    return env, tr


def heldout(pkg, objects=G):
    return pkg.evaluation.HeldOutObjectSet(pkg.CurriculumConfig.variable(), num_heldout_objects=objects, seed=42)


def plan_of(pkg, tr, **kw):
    args = dict(episodes_per_object=K, seed=VAL_SEED, device_seed=DEV_SEED, max_steps=VAL_STEPS)
    args.update(kw)
    return tr.validation_plan(heldout(pkg), **args)


SLAB_FIELDS = ("joint_positions", "joint_velocities", "object_position", "object_velocity", "flags", "step_count",
               "object_size", "object_mass", "friction_coefficient", "curriculum_index", "reset_counter")


def state_of(env, tr):
    torch.cuda.synchronize()
    fields = {f"slab.{k}": getattr(env, k) for k in SLAB_FIELDS}
    fields.update(params=tr.params, m1=tr.m1, m2=tr.m2, packed=tr.packed.view(torch.int16), ep_ret=tr.ep_ret)
    return {k: t.clone() for k, t in fields.items()}


def assert_same_state(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


def sum_bound(x):
    x = np.asarray(x, dtype=np.float64)
    return x.size * EPS * float(np.abs(x).sum())


def records_of(plan):
    torch.cuda.synchronize()
    return dict(ep_return=plan.ep_return.cpu().numpy(), ep_length=plan.ep_length.cpu().numpy(),
                ep_success=plan.ep_success.cpu().numpy(), ep_contacts=plan.ep_contacts.cpu().numpy(),
                status=int(plan.status.item()))


def check_row(row, rec, iteration, env_steps, train_row, solve_threshold=1.0):
    ref = V.row_values(G, K, iteration, env_steps, train_row, rec["ep_return"], rec["ep_length"], rec["ep_success"],
                       rec["ep_contacts"], rec["status"], solve_threshold)
    got = {name: row[k] for k, name in enumerate(V.COLUMNS)}
    for name in ("iteration", "env_steps", "train_row", "episodes", "successes", "success_rate", "mean_length",
                 "mean_contacts", "min_object_success_rate", "objects_solved", "eval_status"):
        assert got[name] == ref[name], name
    if math.isnan(ref["mean_success_length"]):
        assert math.isnan(got["mean_success_length"])
    else:
        assert got["mean_success_length"] == ref["mean_success_length"]
    bound = sum_bound(rec["ep_return"]) / (G * K)
    print("mean_return", got["mean_return"], ref["mean_return"], abs(got["mean_return"] - ref["mean_return"]), bound)
    assert abs(got["mean_return"] - ref["mean_return"]) <= bound
    print("return_std", got["return_std"], ref["return_std"])
    assert abs(got["return_std"] - ref["return_std"]) <= 1e-9 * ref["return_std"]
    return got


# ------------------------------------------------------------------ 1. validation changes nothing
@pytest.mark.parametrize("kw", CONFIGS)
def test_validation_changes_nothing_of_the_training_run(pkg, kw):
    env_t, twin = make(pkg, **kw)
    log_t = twin.fit(4)
    env, tr = make(pkg, **kw)
    log = tr.fit(4, validation=plan_of(pkg, tr), validate_every=2)
    assert_same_state(state_of(env_t, twin), state_of(env, tr))
    assert log.table.tobytes() == log_t.table.tobytes() and log.header == log_t.header
    assert torch.equal(tr._run.best_params, twin._run.best_params)
    assert log_t.validation is None and len(log.validation) == 2
    assert log.validation["iteration"].tolist() == [1.0, 3.0] and log.validation["train_row"].tolist() == [1.0, 3.0]
    assert log.validation["env_steps"].tolist() == [2.0 * tr.M, 4.0 * tr.M]


# ------------------------------------------------------------------ 2. the row is the Evaluator's
@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "stochastic"])
@pytest.mark.parametrize("kw", CONFIGS)
def test_records_are_the_evaluators_and_the_row_their_restatement(pkg, kw, deterministic):
    from dexterous_rl_manipulation_amd import _native as N
    from dexterous_rl_manipulation_amd.trainer import BF
    env, tr = make(pkg, **kw)
    plan = plan_of(pkg, tr, deterministic=deterministic)
    log = tr.fit(2, validation=plan, validate_every=2)
    rec = records_of(plan)
    assert rec["status"] == 0
    # the weights: tr.packed is the pack of tr.params, and the snapshot's actor pack is the same
    fresh = torch.zeros_like(tr.packed)
    N.call("dxrl_pg_pack_weights", tr.dev.index, N.ptr(tr.params), N.ptr(fresh), tr._s())
    torch.cuda.synchronize()
    assert torch.equal(fresh.view(torch.int16), tr.packed.view(torch.int16))
    pol = tr.policy(deterministic=deterministic)
    packed, _, std = pol.device_tensors(tr.dev)
    torch.cuda.synchronize()
    assert torch.equal(packed.view(torch.int16)[:BF["W1c"]], tr.packed.view(torch.int16)[:BF["W1c"]])
    if not deterministic:
        print("std plan", plan.action_std.cpu().numpy(), "snapshot", std.cpu().numpy())
        assert torch.equal(plan.action_std, std)
    ev = pkg.evaluator.Evaluator(pol, heldout(pkg), max_episode_steps=VAL_STEPS)
    res = ev.evaluate_heldout_set(K, VAL_SEED, parallel=True, device_seed=DEV_SEED, return_episodes=True)
    eps = res["all_episodes"]
    assert len(eps) == G * K
    assert [e["episode_steps"] for e in eps] == rec["ep_length"].tolist()
    assert [e["success"] for e in eps] == (rec["ep_success"] != 0).tolist()
    assert [e["num_contacts"] for e in eps] == rec["ep_contacts"].tolist()
    want = np.array([e["episode_reward"] for e in eps], dtype=np.float64)
    assert want.tobytes() == rec["ep_return"].tobytes()  # the same kernel on the same weights and streams
    val = log.validation
    assert len(val) == 1
    got = check_row(val.table[0], rec, 1, 2 * tr.M, 1)
    assert got["episodes"] == G * K and got["success_rate"] == res["overall_stats"]["overall_success_rate"]
    assert val.object_successes[0].tolist() == V.object_successes(G, K, rec["ep_success"]).tolist()
    assert val.object_names == [f"object_{o}" for o in range(G)]
    assert got["is_best"] == 1.0 and val.best_iteration == 1 and val.stopped_iteration is None


# ------------------------------------------------------------------ 3. idempotence
def test_two_runs_of_the_plan_give_identical_records_and_rows(pkg):
    env, tr = make(pkg)
    plan = plan_of(pkg, tr)
    tr.fit(1, validation=plan)
    first = records_of(plan)
    val = tr._run.val
    for _ in range(2):
        plan.run(tr, val, 0, tr.M, 0)
    again = records_of(plan)
    for k in first:
        assert np.array_equal(first[k], again[k]) and np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes(), k
    table = tr.training_log().validation.table
    assert len(table) == 3
    # every column the records determine; is_best / since_best follow the header, which moved on
    assert table[0, :V.IS_BEST].tobytes() == table[1, :V.IS_BEST].tobytes() == table[2, :V.IS_BEST].tobytes()
    objects = tr.training_log().validation.object_successes
    assert objects[0].tolist() == objects[1].tolist() == objects[2].tolist()


# ------------------------------------------------------------------ 4. best model
@pytest.mark.parametrize("kw", CONFIGS)
def test_validation_best_policy_is_the_snapshot_of_its_iteration(pkg, kw):
    """Ten iterations, scored by mean_return: on these trainers the held-out mean return first
    sinks and later jumps above its first value (a2c: rows 0 and 7 are best; ppo2x2: rows 0, 4, 5,
    6), then sinks again, so the best row is neither the first nor the last, and the training
    log's best is iteration 0."""
    env_t, twin = make(pkg, **kw)
    snaps = []
    for _ in range(10):
        twin.iteration()
        torch.cuda.synchronize()
        snaps.append(twin.params.clone())
    env, tr = make(pkg, **kw)
    log = tr.fit(10, validation=plan_of(pkg, tr), validate_every=1, val_keep_best="mean_return")
    val = log.validation
    score = val["mean_return"]
    print("validation mean_return", score.tolist(), "is_best", val["is_best"].tolist(),
          "training mean_return", log["mean_return"].tolist())
    want_rows, want_header, want_table = V.series_rules(score.tolist())
    assert len(want_rows) >= 2  # the case was picked so that the restatement improves more than once
    assert val["is_best"].tolist() == want_table[:, V.IS_BEST].tolist()
    assert val["since_best"].tolist() == want_table[:, V.SINCE_BEST].tolist()
    assert val.header == want_header and val.best_row == want_rows[-1] == int(np.argmax(score))
    b = val.best_iteration
    assert b == want_rows[-1] and 0 < b < 9  # validate_every = 1: row r follows iteration r
    assert torch.equal(tr._run.val.best_params, snaps[b])  # bit for bit
    got, want = tr.best_policy(which="validation"), pkg.policies.MLPActorPolicy.from_params(snaps[b])
    for name in ("W1a", "W2a", "W3a", "logstd"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    # the training-best is kept independently: its own row of the training log, its own buffer
    tb = log.best_iteration
    assert tb == int(np.argmax(log["mean_return"])) and torch.equal(tr._run.best_params, snaps[tb])
    assert tb != b and not torch.equal(tr._run.best_params, tr._run.val.best_params)
    assert tr._run.best_params.data_ptr() != tr._run.val.best_params.data_ptr()
    default = tr.best_policy()
    assert torch.equal(default.W1a, pkg.policies.MLPActorPolicy.from_params(snaps[tb]).W1a)
    with pytest.raises(ValueError):
        tr.best_policy(which="heldout")


# ------------------------------------------------------------------ 5. patience
def sync_debug_mode_works():
    x = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_patience_stops_where_the_restatement_predicts(pkg):
    env_f, full = make(pkg)
    log_f = full.fit(6, validation=plan_of(pkg, full), validate_every=1, val_keep_best="mean_return", patience=1)
    curve = log_f.validation["mean_return"].tolist()
    _, want, _ = V.series_rules(curve, patience=1)
    print("curve", curve, "stopped_row", want["stopped_row"])
    assert len(log_f) == 6 and log_f.validation.header == want  # not stopped without stop_on_patience
    s = want["stopped_row"]
    assert 0 <= s < 5  # the case stops before the run's end
    env, tr = make(pkg)
    log = tr.fit(6, validation=plan_of(pkg, tr), validate_every=1, val_keep_best="mean_return", patience=1,
                 poll_every=1, stop_on_patience=True)
    assert len(log) == s + 1 and tr.iteration_index == s + 1 and tr._run.host_reads == s + 1
    assert log.validation.stopped_iteration == s and len(log.validation) == s + 1
    assert log.validation.table.tobytes() == log_f.validation.table[:s + 1].tobytes()
    with pytest.raises(ValueError):
        tr.fit(1, stop_on_patience=True, patience=1)  # no plan
    with pytest.raises(ValueError):
        tr.fit(1, validation=plan_of(pkg, tr), stop_on_patience=True)  # no patience


def test_fit_with_validation_and_no_polling_reads_nothing(pkg):
    env, tr = make(pkg, **PPO)
    plan = plan_of(pkg, tr, deterministic=False)
    enforced = sync_debug_mode_works()
    print("set_sync_debug_mode('error') enforced by this build:", enforced)
    torch.cuda.set_sync_debug_mode("error")
    try:
        log = tr.fit(3, poll_every=0, validation=plan, validate_every=1, patience=1, stop_on_patience=True)
        reads = tr._run.host_reads
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reads == 0
    assert len(log) == 3 and log.validation["iteration"].tolist() == [0.0, 1.0, 2.0]


# ------------------------------------------------------------------ 6. checkpoints
def test_resume_continues_the_validation_bit_for_bit(pkg, tmp_path):
    settings = dict(validate_every=1, val_keep_best="mean_return", patience=2)
    env_b, b = make(pkg, **PPO)
    log_b = b.fit(4, validation=plan_of(pkg, b), **settings)
    env_a, a = make(pkg, **PPO)
    a.fit(2, validation=plan_of(pkg, a), **settings)
    path = tmp_path / "ck.npz"
    a.save_checkpoint(path)
    env_r = make_env(pkg)
    r = pkg.trainer.PGTrainer.load_checkpoint(path, env_r)
    assert r._run.val is not None and r._run.val.rows == 2
    with pytest.raises(ValueError, match="seed"):
        r.fit(1, validation=plan_of(pkg, r, seed=VAL_SEED + 1), **settings)
    with pytest.raises(ValueError, match="episodes_per_object"):
        r.fit(1, validation=plan_of(pkg, r, episodes_per_object=K + 1), **settings)
    assert r.iteration_index == 2  # a refused plan ran nothing
    log_r = r.fit(2, validation=plan_of(pkg, r), **settings)
    assert_same_state(state_of(env_b, b), state_of(env_r, r))
    assert log_r.table.tobytes() == log_b.table.tobytes() and log_r.header == log_b.header
    vr, vb = log_r.validation, log_b.validation
    assert len(vr) == 4 and vr.table.tobytes() == vb.table.tobytes() and vr.header == vb.header
    assert np.array_equal(vr.object_successes, vb.object_successes) and vr.object_names == vb.object_names
    assert torch.equal(r._run.val.best_params, b._run.val.best_params)
    assert torch.equal(r._run.best_params, b._run.best_params)
    # a second plan on the same trainer is refused too, and a run never validated checkpoints as before
    with pytest.raises(ValueError, match="max_steps"):
        b.fit(1, validation=plan_of(pkg, b, max_steps=VAL_STEPS + 1))
    env_p, p = make(pkg)
    p.fit(1)
    plain = tmp_path / "plain.npz"
    p.save_checkpoint(plain)
    arrays, meta = pkg.training_run.read_checkpoint(plain)
    assert "validation" not in meta and not any(k.startswith("val_") for k in arrays)
    q = pkg.trainer.PGTrainer.load_checkpoint(plain, make_env(pkg))
    assert q._run.val is None and q.training_log().validation is None
    log_q = q.fit(1, validation=plan_of(pkg, q))  # and may start validating after the load
    assert len(log_q) == 2 and len(log_q.validation) == 1 and log_q.validation["iteration"].tolist() == [1.0]


def test_too_many_objects_and_collective_trainers_raise(pkg):
    env, tr = make(pkg)
    with pytest.raises(ValueError, match="256"):
        tr.validation_plan(heldout(pkg, objects=257), episodes_per_object=1)
    with pytest.raises(ValueError):
        tr.validation_plan(heldout(pkg), episodes_per_object=0)
    with pytest.raises(ValueError):
        tr.fit(1, validation=object())
    with pytest.raises(ValueError):
        tr.fit(1, validation=plan_of(pkg, tr), val_keep_best="is_best")
    assert tr.iteration_index == 0
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        env_c = make_env(pkg)
        col = pkg.trainer.PGTrainer(env_c, pkg.trainer.TrainerConfig(horizon=16, seed=1),
                                    process_group=dist.group.WORLD, world_size=1)
        with pytest.raises(ValueError, match="one rank"):
            col.fit(1, validation=plan_of(pkg, tr))
        assert col.iteration_index == 0
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ 7. the CLI, in a child process
def test_cli_child_process_writes_the_validation_files(pkg, tmp_path):
    from dexterous_rl_manipulation_amd import train, training_run
    common = ["--config-name", "easy", "--envs", "128", "--horizon", "16", "--max-steps", "12", "--iterations", "3",
              "--validate-every", "1", "--val-episodes", "2", "--val-seed", "7", "--val-keep-best", "mean_return"]
    here = tmp_path / "here"
    assert train.main(common + ["--out", str(here)]) == 0
    child = tmp_path / "child"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-m", "dexterous_rl_manipulation_amd.train"] + common + ["--out", str(child)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("training_log.json", "best_policy.npz", "checkpoint.npz", "best_val_policy.npz"):
        assert (child / name).exists(), name
    log_c = training_run.TrainingLog.load(child / "training_log.json")
    log_h = training_run.TrainingLog.load(here / "training_log.json")
    vc, vh = log_c.validation, log_h.validation
    assert len(vc) == 3 and vc["iteration"].tolist() == [0.0, 1.0, 2.0] and vc["episodes"].tolist() == [40.0] * 3
    assert vc.table.tobytes() == vh.table.tobytes() and vc.header == vh.header
    assert np.array_equal(vc.object_successes, vh.object_successes) and len(vc.object_names) == 20
    pol = pkg.policies.MLPActorPolicy.load(child / "best_val_policy.npz")
    assert pol.W1a.shape == (256, 64) and vc.best_row is not None
    arrays, meta = training_run.read_checkpoint(child / "checkpoint.npz")
    assert meta["validation"]["rows"] == 3 and arrays["val_table"].shape == (3, V.COLS)
