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
CONFIG_DEFAULTS = {"value_norm": False, "value_norm_eps": 1e-5}


def validate_value_norm(cfg) -> None:
    """ValueError for a value-normalisation configuration that cannot do what it says."""
    eps = cfg.value_norm_eps
    if not (isinstance(eps, (int, float)) and math.isfinite(eps) and eps >= 0.0):
        raise ValueError(f"value_norm_eps must be finite and >= 0, got {eps!r}")


def check_checkpoint(value_norm: bool, has_block: bool, path="checkpoint") -> None:
    """A checkpoint carries the state block iff its trainer_config sets value_norm: ValueError
    otherwise (a critic trained in normalised units cannot continue without its moments, and a
    plain critic has none to continue from)."""
    if value_norm and not has_block:
        raise ValueError(f"{path}: trainer_config sets value_norm and the file has no value_norm_state block")
    if has_block and not value_norm:
        raise ValueError(f"{path}: the file carries a value_norm_state block and trainer_config does not set "
                         "value_norm")


def state_dict(block) -> Dict[str, float]:
    """The block's words (a sequence of PG_VNORM_WORDS floats) as value_norm_state() returns them."""
    from ._native import PG_VNORM as W
    b = [float(x) for x in block]
    var = lambda n, m2: math.sqrt(m2 / n) if n > 0.0 else 0.0  # noqa: E731  (population, as sigma is)
    return {"count": b[W["count"]], "mean": b[W["mean"]], "std": var(b[W["count"]], b[W["m2"]]),
            "mu": b[W["mu"]], "sigma": b[W["sigma"]], "batch_mean": b[W["batch_mean"]],
            "batch_std": var(b[W["batch_count"]], b[W["batch_m2"]]), "calls": int(b[W["calls"]])}
