"""Kernel time of the evaluation episode programs with the frozen MLP actor (k_eval_mlp) beside the
frozen SimpleLearner (k_eval_ls) on the same held-out plan: 10 objects x K episodes, one lane per
episode, device Philox streams.  One JSON line per policy and round.

    python tools/eval_mlp_bench.py [--episodes-per-object 4096] [--config hard]
                                   [--policies simple,mlp_det,mlp_sto] [--rounds 3] [--root DIR]

--root: the checkout whose package is measured (default: this one), so the SIMPLE yardstick can be
taken on another commit's tree with the same script.  kernel_ms is the HIP-event time per launch
(EpisodeProgram.run(timing=...), 20 back-to-back launches after a warm-up launch).  MFMA work:
each workgroup step runs the actor on a 16-row tile, 16 x 161,792 FLOP (2 x (64 x 256 + 256 x 256 +
256 x 16) per row), whether or not all 16 rows hold a running episode; the env-step figure
(env_steps x 161,792 FLOP) is the useful part of it."""
import argparse
import json
import os
import sys

import numpy as np

ROW_FLOP = 2 * (64 * 256 + 256 * 256 + 256 * 16)  # 161,792
PEAK_BF16 = 16 * 157.3e12  # dense BF16 MFMA peak (MI355X: 16 x the FP32 rate)
MEAN = [-0.3, -0.2, -0.1, 0.1, 0.2, 0.3, -0.4, -0.4, 0.0, 0.25, -0.25, 0.1, -0.1, 0.05, -0.05]


class Frozen:
    exploration_noise = 0.3
    mean_action = np.asarray(MEAN, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes-per-object", type=int, default=4096)
    ap.add_argument("--config", default="hard")
    ap.add_argument("--policies", default="simple,mlp_det,mlp_sto")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    ap.add_argument("--head-gain", type=float, default=2.0,
                    help="gain of the actor's head initialisation (0: mu = 0 whatever the observation)")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import evaluation as ev, evaluator as evr

    def actor(deterministic):
        # the trainer's initialisation with a head gain of 2 by default (actions that depend on the observation)
        import math
        import torch
        from dexterous_rl_manipulation_amd.policies import MLPActorPolicy
        g = torch.Generator(device="cpu").manual_seed(0)
        w = {}
        for name, rows, cols, gain in (("W1a", 256, 45, math.sqrt(2)), ("W2a", 256, 256, math.sqrt(2)),
                                       ("W3a", 15, 256, a.head_gain)):
            w[name] = torch.empty(rows, cols)
            torch.nn.init.orthogonal_(w[name], gain=gain, generator=g)
        W1, W2, W3 = torch.zeros(256, 64), torch.zeros(256, 288), torch.zeros(32, 288)
        W1[:, :45], W2[:, :256], W3[:15, :256] = w["W1a"], w["W2a"], w["W3a"]
        return MLPActorPolicy(W1, W2, W3, torch.full((15,), -0.5), deterministic=deterministic, seed=0)

    h = ev.HeldOutObjectSet(getattr(pkg.CurriculumConfig, a.config)(), num_heldout_objects=10, seed=42)
    for rnd in range(a.rounds):
        for name in a.policies.split(","):
            pol = Frozen() if name == "simple" else actor(name == "mlp_det")
            e = ev.Evaluator(pol, h, max_episode_steps=a.max_episode_steps)
            prog = evr.policy_program(pol)
            p = e.heldout_program(a.episodes_per_object, 0, parallel=True)
            kw = dict(host_resets=False, host_noise=False, keep_history=False)
            p.run(prog, **kw)  # warm
            t = {}
            rec = p.run(prog, repeat=20, timing=t, **kw)
            steps = int(rec.ep_length.astype(np.int64).sum())
            E, sec = len(rec.ep_length), t["kernel_ms"] * 1e-3
            out = {"label": a.label, "round": rnd, "policy": name, "head_gain": a.head_gain, "config": a.config,
                   "episodes": E, "env_steps": steps, "mean_length": steps / E, "success_rate": float(rec.ep_success.mean()),
                   "kernel_ms": round(t["kernel_ms"], 4), "env_steps_per_s": steps / sec,
                   "episodes_per_s": E / sec}
            if name != "simple":
                out["useful_mfma_tflops"] = steps * ROW_FLOP / sec / 1e12
                out["useful_mfma_share_of_bf16_peak"] = steps * ROW_FLOP / sec / PEAK_BF16
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
