"""Worker for tests/test_gpu_sharded_fit.py (not collected by pytest): one rank of a sharded
PGTrainer training run on cuda:0 over gloo.  Rank r owns envs [r*n, (r+1)*n) of the global batch,
as tests/dist_pg_worker.py shards them.

    python tests/sharded_fit_worker.py fit OUT.pt N_LOCAL CONFIG       (RANK / WORLD_SIZE / MASTER_* in env)
    python tests/sharded_fit_worker.py resume OUT.pt N_LOCAL DIR

fit:    fit(3, merge_ranks=True, converge=...) on config `variable` or `default`; saves the log, the
        header, the best parameters, the per-rank records and the last iteration's tape.  At world 1
        (no process group) the three iterations run as fit(1) + fit(2) on the same log, and the first
        iteration's tape is saved too.
resume: config `default` with its scheduler and a small validation plan, both in this process: an
        uninterrupted fit(4), and fit(2) + save_checkpoint + load_checkpoint + fit(2); saves both
        runs' parameters, Adam moments, log, header and validation table.
"""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HORIZON, MAX_STEPS = 32, 40
CONVERGE = ("mean_return", 2, -1e9)


def setup():
    import torch
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    group = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))  # ranks share the one test GPU
        group = dist.group.WORLD
    return world, rank, dev, group


def make_env(n, rank, dev, config):
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import envs
    cur = {"default": "easy"}.get(config, config)
    return envs.VecEnv(n, curriculum_config=pkg.CurriculumConfig.named(cur), reward_type="dense", seed=99, device=dev,
                       global_env_offset=rank * n)


def make(n, rank, world, dev, group, config):
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import trainer
    env = make_env(n, rank, dev, config)
    cfg = trainer.TrainerConfig(horizon=HORIZON, seed=4, ent_coef=0.01, max_steps=MAX_STEPS,
                                record_cap=32 if config == "default" else 0)
    tr = trainer.PGTrainer(env, cfg, process_group=group, world_size=world)
    if config == "default":
        C = pkg.CurriculumConfig
        tr.attach_curriculum(pkg.experiments.CurriculumScheduler(C.easy(), C.hard(), 0.3, 20, 15, 5))
    env.reset(write_obs=False)
    return env, tr


def tape(tr):
    """What pg_log_reference.row_values reads of the iteration that just ran."""
    import torch
    torch.cuda.synchronize()
    host = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    return dict(n=tr.n, T=tr.T, rew=host(tr.rew), ret=host(tr.ret), done=host(tr.done), values=host(tr.V[0])[:tr.M],
                ep_count=host(tr.ep_count), ep_sum_return=host(tr.ep_sum_ret), ep_sum_length=host(tr.ep_sum_len),
                ep_successes=host(tr.ep_succ), loss_partial=host(tr.fused_loss), loss_rows=int(tr._loss_rows),
                stats=host(tr.stats), gnorm2=float(tr.gnorm2.item()))


def run_state(tr, log):
    import torch
    torch.cuda.synchronize()
    st = tr._run
    out = dict(table=log.table.copy(), header=st.header.cpu().numpy().copy(), header_dict=dict(log.header),
               best_params=st.best_params.cpu().numpy().copy(), ranks=log.ranks.copy(),
               params=tr.params.cpu().numpy().copy(), m1=tr.m1.cpu().numpy().copy(), m2=tr.m2.cpu().numpy().copy(),
               env_steps=st.env_steps)
    if log.validation is not None:
        out.update(val_table=log.validation.table.copy(), val_header=st.val.header.cpu().numpy().copy(),
                   val_best_params=st.val.best_params.cpu().numpy().copy(),
                   val_objects=log.validation.object_successes.copy())
    return out


def finish(res, out, world, group):
    import torch
    torch.save(res, out)
    if world > 1:
        import torch.distributed as dist
        dist.barrier(group=group)
        dist.destroy_process_group()


def fit(out, n, config):
    world, rank, dev, group = setup()
    _, tr = make(n, rank, world, dev, group, config)
    res = {}
    if world == 1:
        tr.fit(1, merge_ranks=True, converge=CONVERGE)
        res["tape0"] = tape(tr)
        log = tr.fit(2, merge_ranks=True, converge=CONVERGE)
    else:
        log = tr.fit(3, merge_ranks=True, converge=CONVERGE)
    res.update(run_state(tr, log), tape=tape(tr))
    finish(res, out, world, group)


def resume(out, n, ckdir):
    from dexterous_rl_manipulation_amd import trainer
    from dexterous_rl_manipulation_amd.evaluation import HeldOutObjectSet
    world, rank, dev, group = setup()

    def run(tr, iterations):
        # the held-out set of the run's own config (the scheduler moves the env's afterwards), as train.py builds it
        plan = tr.validation_plan(HeldOutObjectSet(base), episodes_per_object=2, max_steps=MAX_STEPS)
        return tr.fit(iterations, merge_ranks=True, converge=CONVERGE, validation=plan, validate_every=2)

    env_b, b = make(n, rank, world, dev, group, "default")
    base = env_b.curriculum_configs[0]
    straight = run_state(b, run(b, 4))
    env_a, a = make(n, rank, world, dev, group, "default")
    run(a, 2)
    path = os.path.join(ckdir, f"checkpoint.rank{rank}.npz")
    a.save_checkpoint(path)
    refused = ""
    try:
        trainer.PGTrainer.load_checkpoint(path, make_env(n, rank, dev, "default"), world_size=1)
    except ValueError as e:
        refused = str(e)
    env_r = make_env(n, rank, dev, "default")
    r = trainer.PGTrainer.load_checkpoint(path, env_r, process_group=group, world_size=world)
    assert r is not a and r.collective and r.iteration_index == 2
    resumed = run_state(r, run(r, 2))
    finish(dict(straight=straight, resumed=resumed, refused=refused, sched=(b.scheduler.get_state(), r.scheduler.get_state())),
           out, world, group)


if __name__ == "__main__":
    mode, out, n, arg = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    {"fit": fit, "resume": resume}[mode](out, n, arg)
