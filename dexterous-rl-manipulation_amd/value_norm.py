"""Value normalisation of ``PGTrainer``: the host side of ``dxrl_pg_gae_vnorm``.

The critic learns in normalised units; the advantages launch decodes its outputs and encodes its
targets with running return moments kept in a device block (include/dxrl.h states the arithmetic).
What the host contributes is pure and small: the checks of a configuration, the checkpoint rule,
and the block read back as a dict.
"""
from __future__ import annotations

import math
from typing import Dict

# the TrainerConfig fields of this layer, with the defaults that reproduce a trainer without it
CONFIG_DEFAULTS = {"value_norm": False, "value_norm_eps": 1e-5, "popart": False, "value_norm_forget": 0.0}


def validate_value_norm(cfg) -> None:
    """ValueError for a value-normalisation configuration that cannot do what it says."""
    eps = cfg.value_norm_eps
    if not (isinstance(eps, (int, float)) and math.isfinite(eps) and eps >= 0.0):
        raise ValueError(f"value_norm_eps must be finite and >= 0, got {eps!r}")
    on = bool(getattr(cfg, "value_norm", False))
    forget = getattr(cfg, "value_norm_forget", 0.0)
    if not (isinstance(forget, (int, float)) and math.isfinite(forget) and 0.0 <= forget < 1.0):
        raise ValueError(f"value_norm_forget must be in [0, 1), got {forget!r}")
    if forget > 0.0 and not on:
        raise ValueError("value_norm_forget > 0 needs value_norm: the forgetting factor acts on its running moments")
    if getattr(cfg, "popart", False) and not on:
        raise ValueError("popart needs value_norm: it rescales the critic's head when value_norm's (mu, sigma) move")


def check_checkpoint(value_norm: bool, has_block: bool, path="checkpoint") -> None:
    """A checkpoint carries the state block iff its trainer_config sets value_norm: ValueError
    otherwise (a critic trained in normalised units cannot continue without its moments, and a
    plain critic has none to continue from)."""
    if value_norm and not has_block:
        raise ValueError(f"{path}: trainer_config sets value_norm and the file has no value_norm_state block")
    if has_block and not value_norm:
        raise ValueError(f"{path}: the file carries a value_norm_state block and trainer_config does not set "
                         "value_norm")


def check_popart_checkpoint(popart: bool, has_block: bool, path="checkpoint") -> None:
    """Likewise for the popart block: without it the head's units are unknown, and a trainer
    without popart never rescales a head whose units differ from the block's."""
    if popart and not has_block:
        raise ValueError(f"{path}: trainer_config sets popart and the file has no popart_state block")
    if has_block and not popart:
        raise ValueError(f"{path}: the file carries a popart_state block and trainer_config does not set popart")


def check_forget(forget: float, block, path="checkpoint") -> None:
    """The FORGET word of a stored value_norm_state block is the configuration's factor."""
    from ._native import PG_VNORM as W
    word = float(block[W["forget"]])
    if word != float(forget):
        raise ValueError(f"{path}: the value_norm_state block was folded with a forgetting factor of {word!r} and "
                         f"trainer_config sets value_norm_forget = {float(forget)!r}")


def popart_dict(block) -> Dict[str, float]:
    """The popart block's words (PG_POPART_WORDS floats) as popart_state() returns them."""
    from ._native import PG_POPART as W
    b = [float(x) for x in block]
    return {"mu_head": b[W["mu_head"]], "sigma_head": b[W["sigma_head"]], "rescales": int(b[W["rescales"]]),
            "skipped": int(b[W["skipped"]]), "last_scale": b[W["last_scale"]], "last_shift": b[W["last_shift"]]}


def state_dict(block) -> Dict[str, float]:
    """The block's words (a sequence of PG_VNORM_WORDS floats) as value_norm_state() returns them."""
    from ._native import PG_VNORM as W
    b = [float(x) for x in block]
    var = lambda n, m2: math.sqrt(m2 / n) if n > 0.0 else 0.0  # noqa: E731  (population, as sigma is)
    return {"count": b[W["count"]], "mean": b[W["mean"]], "std": var(b[W["count"]], b[W["m2"]]),
            "mu": b[W["mu"]], "sigma": b[W["sigma"]], "batch_mean": b[W["batch_mean"]],
            "batch_std": var(b[W["batch_count"]], b[W["batch_m2"]]), "calls": int(b[W["calls"]])}
