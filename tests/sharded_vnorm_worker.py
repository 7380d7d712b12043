"""Worker for tests/test_gpu_vnorm_run.py (not collected by pytest): one rank of a sharded PGTrainer
with value normalisation on cuda:0 over gloo, set up as tests/sharded_fit_worker.py sets its ranks up.

    python tests/sharded_vnorm_worker.py OUT.pt N_LOCAL       (RANK / WORLD_SIZE / MASTER_* in env)

Two iterations on the hard curriculum.  After each: the state block, the gathered rows [world][6]
(row r: rank r's own return and advantage triples, as its dxrl_pg_gae_vnorm call left them), the
combined statistics and this rank's raw returns."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sharded_fit_worker import finish, setup  # noqa: E402

HORIZON, MAX_STEPS = 40, 8


def main(out, n):
    import torch

    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import envs, trainer
    world, rank, dev, group = setup()
    env = envs.VecEnv(n, curriculum_config=pkg.CurriculumConfig.hard(), reward_type="dense", seed=3, device=dev,
                      global_env_offset=rank * n)
    cfg = trainer.TrainerConfig(horizon=HORIZON, seed=1, ent_coef=0.01, max_steps=MAX_STEPS, value_norm=True)
    tr = trainer.PGTrainer(env, cfg, process_group=group, world_size=world)
    env.reset(write_obs=False)
    res = {"iterations": []}
    for _ in range(2):
        tr.iteration()
        torch.cuda.synchronize()
        res["iterations"].append({k: getattr(tr, k).cpu().clone() for k in ("vnorm", "moments_all", "stats", "ret")})
    res["state"] = tr.value_norm_state()
    res["params"] = tr.params.cpu().clone()
    finish(res, out, world, group)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
