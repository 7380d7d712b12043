"""Worker for tests/test_gpu_popart_run.py (not collected by pytest): one rank of a sharded PGTrainer
with value normalisation, a forgetting factor and PopArt on cuda:0 over gloo, set up as
tests/sharded_fit_worker.py sets its ranks up.

    python tests/sharded_popart_worker.py OUT.pt N_LOCAL       (RANK / WORLD_SIZE / MASTER_* in env)

Two iterations on the hard curriculum; then the parameters, the pack and both state blocks."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sharded_fit_worker import finish, setup  # noqa: E402
from sharded_vnorm_worker import HORIZON, MAX_STEPS  # noqa: E402

FORGET = 0.05


def main(out, n):
    import torch

    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import envs, trainer
    world, rank, dev, group = setup()
    env = envs.VecEnv(n, curriculum_config=pkg.CurriculumConfig.hard(), reward_type="dense", seed=3, device=dev,
                      global_env_offset=rank * n)
    cfg = trainer.TrainerConfig(horizon=HORIZON, seed=1, ent_coef=0.01, max_steps=MAX_STEPS, value_norm=True,
                                popart=True, value_norm_forget=FORGET)
    tr = trainer.PGTrainer(env, cfg, process_group=group, world_size=world)
    env.reset(write_obs=False)
    for _ in range(2):
        tr.iteration()
    torch.cuda.synchronize()
    res = {k: getattr(tr, k).cpu().clone() for k in ("params", "vnorm", "popart")}
    res["packed"] = tr.packed.view(torch.int16).cpu().clone()
    res["popart_state"], res["value_norm_state"] = tr.popart_state(), tr.value_norm_state()
    finish(res, out, world, group)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
