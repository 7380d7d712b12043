"""Step-size control of ``PGTrainer``: the host side of ``dxrl_pg_adam_step_ctl``.

The decisions (KL stop, KL-adaptive scale, Adam's t) are taken inside the optimiser launch from a
device state block; what the host contributes is pure and small: whether the control path runs at
all, the checks of a configuration, and the nominal learning rate of an iteration -- an f64
function of the iteration index alone, so a resumed run recomputes it.
"""
from __future__ import annotations

import math

SCHEDULES = ("constant", "linear", "cosine")
# the TrainerConfig fields of this layer, with the defaults that reproduce a trainer without it
CONFIG_DEFAULTS = {"lr_schedule": "constant", "lr_final": None, "lr_schedule_iterations": None, "target_kl": None,
                   "kl_stop": True, "kl_stop_factor": 1.5, "kl_adaptive": False, "kl_adapt_factor": 1.5,
                   "kl_adapt_band": 2.0, "lr_min": 1e-6, "lr_max": 1e-2}


def control_enabled(cfg) -> bool:
    """The control path runs with a non-constant schedule or a target KL."""
    return cfg.lr_schedule != "constant" or cfg.target_kl is not None


def validate_lr_control(cfg) -> None:
    """ValueError for a step-size configuration that cannot do what it says."""
    if cfg.lr_schedule not in SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {list(SCHEDULES)}, got {cfg.lr_schedule!r}")
    if not control_enabled(cfg):
        if cfg.kl_adaptive:
            raise ValueError("kl_adaptive needs target_kl: the KL it steers the learning rate towards")
        return
    if not (math.isfinite(cfg.lr) and cfg.lr > 0.0):
        raise ValueError(f"lr must be finite and > 0, got {cfg.lr}")
    if not (0.0 < cfg.lr_min <= cfg.lr_max and math.isfinite(cfg.lr_max)):
        raise ValueError(f"need 0 < lr_min <= lr_max, got lr_min={cfg.lr_min} > lr_max={cfg.lr_max}"
                         if cfg.lr_min > cfg.lr_max else
                         f"need finite 0 < lr_min <= lr_max, got lr_min={cfg.lr_min}, lr_max={cfg.lr_max}")
    if cfg.lr_schedule != "constant":
        if cfg.lr_final is None or cfg.lr_schedule_iterations is None:
            raise ValueError(f"lr_schedule={cfg.lr_schedule!r} needs lr_final and lr_schedule_iterations")
        if not (math.isfinite(cfg.lr_final) and cfg.lr_final > 0.0) or int(cfg.lr_schedule_iterations) < 1:
            raise ValueError("lr_final must be finite and > 0 and lr_schedule_iterations >= 1")
    if cfg.kl_adaptive and cfg.target_kl is None:
        raise ValueError("kl_adaptive needs target_kl: the KL it steers the learning rate towards")
    if cfg.target_kl is not None:
        if not (math.isfinite(cfg.target_kl) and cfg.target_kl > 0.0):
            raise ValueError(f"target_kl must be finite and > 0, got {cfg.target_kl}")
        if cfg.epochs * cfg.minibatches == 1:
            raise ValueError("target_kl with epochs x minibatches == 1: the only pass of an iteration runs on the "
                             "rollout's own weights (ratio 1, KL 0), so no rule could ever act")
        if cfg.kl_adaptive and cfg.epochs < 2:
            raise ValueError("kl_adaptive needs epochs >= 2: the last epoch's KL is measured against a policy that "
                             "an earlier epoch has moved")
        if not cfg.fused:
            raise ValueError("a KL rule needs the fused learner (fused=True): the GEMM chain's loss partials are not "
                             "wired to the optimiser step")
        if not (cfg.kl_stop_factor > 0.0 and cfg.kl_adapt_factor > 1.0 and cfg.kl_adapt_band >= 1.0):
            raise ValueError("need kl_stop_factor > 0, kl_adapt_factor > 1 and kl_adapt_band >= 1")


def lr_nominal(cfg, iteration: int) -> float:
    """The schedule's learning rate of iteration `iteration` (f64): cfg.lr at 0, cfg.lr_final at
    lr_schedule_iterations and held beyond it."""
    lr = float(cfg.lr)
    if cfg.lr_schedule == "constant":
        return lr
    n, i, end = int(cfg.lr_schedule_iterations), int(iteration), float(cfg.lr_final)
    if i <= 0:
        return lr
    if i >= n:
        return end
    if cfg.lr_schedule == "linear":
        return lr + (end - lr) * (i / n)
    return end + 0.5 * (lr - end) * (1.0 + math.cos(math.pi * i / n))
