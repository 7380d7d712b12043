"""CPU restatement of one curriculum training run, composed from the oracle
(oracle/dx_oracle.py: OracleEnv, OracleSimpleLearner, reset_draws) and the host schedulers
(experiments.CurriculumScheduler / StepBasedScheduler .update):

    evaluation/curriculum_ablation.py:62-73
        success, steps, reward = run_episode(env, policy)
        if scheduler.update(success, steps): env.curriculum_config = scheduler.get_current_config()

with the env's gymnasium stream seeded by ``env_seed`` and the learner's np.random stream by
``learner_seed``.  ``success_rule="terminated"`` feeds the scheduler ``terminated`` of the
episode's last step (evaluator.py:157); "training" feeds False (episode_utils.py:52)."""
import copy

import numpy as np

from oracle.dx_oracle import OracleCurriculum, OracleEnv, OracleSimpleLearner, reset_draws


def to_oracle(cfg) -> OracleCurriculum:
    return OracleCurriculum(object_size=cfg.object_size, object_mass=cfg.object_mass,
                            friction_coefficient=cfg.friction_coefficient, size_range=cfg.object_size_range,
                            mass_range=cfg.object_mass_range, friction_range=cfg.friction_range,
                            spawn_x_range=cfg.spawn_x_range, spawn_y_range=cfg.spawn_y_range,
                            spawn_z_range=cfg.spawn_z_range,
                            friction_is_np_float64=(cfg.friction_range is None
                                                    and isinstance(cfg.friction_coefficient, np.floating)))


def curriculum_run(proto, learner_seed: int, env_seed: int, num_episodes: int, max_steps: int, dense: bool = True,
                   success_rule: str = "terminated", learning_rate: float = 0.01):
    """Returns per-episode lists: rewards, steps, successes, difficulty levels (after the update)."""
    s = copy.deepcopy(proto)
    s.reset()
    if hasattr(s, "current_milestone_idx"):
        s.current_milestone_idx = 0
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(env_seed))))
    gauss = np.random.RandomState(int(learner_seed)).standard_normal(2 * 15 * num_episodes * max_steps)
    env = OracleEnv(cur=to_oracle(s.get_current_config()), dense=dense, max_episode_steps=max_steps)
    pol = OracleSimpleLearner(gauss, learning_rate=learning_rate)
    rewards, steps, successes, levels = [], [], [], []
    for ep in range(num_episodes):
        env.reset(reset_draws(rng, env.cur, first=ep == 0))
        pol.reset()
        total, term, step = 0.0, False, 0
        for step in range(max_steps):
            _, r, term, trunc = env.step(pol.select_action())
            total += r
            pol.update(r)
            if term or trunc:
                break
        success = bool(term) if success_rule == "terminated" else False
        if s.update(success, step + 1):
            env.cur = to_oracle(s.get_current_config())
        rewards.append(total)
        steps.append(step + 1)
        successes.append(success)
        levels.append(float(s.get_difficulty_level()))
    return rewards, steps, successes, levels
