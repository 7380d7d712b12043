"""Training runs of ``PGTrainer``: ``fit`` with a learning curve kept on the device, keep-best,
a convergence rule, and checkpoints.

``fit`` calls ``PGTrainer.iteration()`` and then ``dxrl_pg_log_row`` (csrc/dxrl_pg_log.hip), which
reduces what the iteration left on the device into one f64 row of a device table and applies the
keep-best and convergence rules to a small device header.  Nothing returns to the host until the
run is over (``poll_every=0``): the returned ``TrainingLog`` is filled by one asynchronous copy
that is waited for when a column is first read.

A checkpoint is one ``.npz`` without pickle -- arrays plus one JSON string, in the style of
``MLPActorPolicy.save`` -- holding everything a resumed run needs to continue bit for bit: the
master parameters, Adam moments, bf16 pack and counters, the running episode returns, the env
slab (offsets only, nothing address-dependent), the curriculum table's configs, the trainer
config, the log table / header / best parameters, and the attached scheduler.

``fit(validation=plan)`` adds held-out validation: a ``ValidationPlan`` built once (the launch of
``Evaluator.evaluate_heldout_set(parallel=True)`` with device Philox resets) runs the episode
kernel on the trainer's live weights every ``validate_every`` iterations, and ``dxrl_pg_val_row``
(csrc/dxrl_pg_val.hip) reduces its episode records to one row of a second device table with its
own keep-best, best parameters and patience.  ``log.validation`` is the ``ValidationLog``; the
checkpoint carries the validation tables and the plan's fingerprint as optional entries.

A plan built with ``noise_levels`` validates under every (obs_std, dyn_std) level in the one
episode launch, and ``dxrl_pg_val_levels_row`` (csrc/dxrl_pg_val_levels.hip) writes the clean
row, a row per level with the degradation columns, and a row of scores over the levels
(worst / mean success rate, worst mean return) that keep-best and patience may follow.  With
``common_random_numbers`` the episode launch runs with ``stream_period = G K``, so every level
replays the baseline's episodes under its own noise scale, and ``dxrl_pg_val_paired_row``
(csrc/dxrl_pg_val_paired.hip) adds a paired table: per level the episodes lost and gained against
the baseline and the mean and error of the per-episode return difference.  With ``failure_modes``
the episode launch also accumulates the five history words of every episode, and
``dxrl_pg_val_failure_row`` (csrc/dxrl_pg_val_failure.hip) classifies every episode with the failure
taxonomy and adds, per level, a table of the modes, a row of totals and -- with common random
numbers -- the class transitions against the baseline.

``fit(merge_ranks=True)`` is the run of a sharded (collective) trainer: per logged iteration
``dxrl_pg_log_rank_pack`` reduces the rank's tape to one record, the records are all-gathered, and
``dxrl_pg_log_row_world`` finishes the row from all of them, so every rank holds the same table,
header and best parameters; ``log.ranks`` keeps the records, and each rank checkpoints its own file.

On a trainer with step-size control (``TrainerConfig.lr_schedule`` / ``target_kl``) the run keeps a
third device table, ``log.optimizer``: the last ``dxrl_pg_adam_step_ctl`` launch of every iteration
writes the iteration's row (learning rate, updates applied / skipped, stop pass, KLs, next scale)
straight into it.  The table and the trainer's device state block ride the JSON and the checkpoint
as optional entries.

On a trainer with ``TrainerConfig.popart`` the run likewise keeps ``log.value_norm``: the
``dxrl_pg_popart_rescale`` launch that ends every iteration writes the row (the new and the previous
(mu, sigma), the head's scale and shift, the running and the batch moments).  ``value_mse`` of the
main table is in normalised units under ``value_norm``; ``sigma`` of this table is the factor.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import weakref
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _native as N

COLUMNS = N.PG_LOG_COLUMNS
COLS = N.PG_LOG_COLS
CHECKPOINT_FORMAT = "dxrl-pg-checkpoint-v1"
LOG_FORMAT = "dxrl-training-log-v1"
_SCORE_COLUMNS = COLUMNS[:N.PG_LOG_IS_BEST]  # columns a score / convergence rule may read
_HEADER_BYTES = C.sizeof(N.PgLogHeader)
RANK_COLUMNS = N.PG_LOG_RANK_COLUMNS    # the named entries of a rank record (fit(merge_ranks=True))
RANK_DOUBLES = N.PG_LOG_RANK_DOUBLES
_MIN_CAP = 256
OPT_COLUMNS = N.PG_OPT_COLUMNS          # the named columns of log.optimizer (step-size control)
VNORM_COLUMNS = N.PG_VNORM_LOG_COLUMNS  # the named columns of log.value_norm (popart)
VNORM_COLS = N.PG_VNORM_LOG_COLS
OPT_COLS = N.PG_OPT_COLS
VAL_COLUMNS = N.PG_VAL_COLUMNS
VAL_COLS = N.PG_VAL_COLS
_VAL_SCORE_COLUMNS = VAL_COLUMNS[:N.PG_VAL_IS_BEST]  # columns the validation keep-best may read
_VAL_HEADER_BYTES = C.sizeof(N.PgValHeader)
_MIN_VAL_CAP = 64
VAL_LEVEL_COLUMNS = N.PG_VAL_LEVEL_COLUMNS
VAL_LEVEL_COLS = N.PG_VAL_LEVEL_COLS
VAL_ROBUST_COLUMNS = N.PG_VAL_ROBUST_COLUMNS
VAL_ROBUST_COLS = N.PG_VAL_ROBUST_COLS
VAL_PAIRED_COLUMNS = N.PG_VAL_PAIRED_COLUMNS
VAL_PAIRED_COLS = N.PG_VAL_PAIRED_COLS
VAL_FAILURE_MODE_COLUMNS = N.PG_VAL_FAILURE_MODE_COLUMNS
VAL_FAILURE_MODE_COLS = N.PG_VAL_FAILURE_MODE_COLS
VAL_FAILURE_LEVEL_COLUMNS = N.PG_VAL_FAILURE_LEVEL_COLUMNS
VAL_FAILURE_LEVEL_COLS = N.PG_VAL_FAILURE_LEVEL_COLS
# list(FailureMode) order, as ep_mode has it; the classes of the transitions: success, then the modes
FAILURE_MODE_NAMES = ("slippage", "unstable_grasp", "misalignment", "timeout", "object_dropped",
                      "insufficient_contacts")
FAILURE_CLASS_NAMES = ("success",) + FAILURE_MODE_NAMES
_MODES, _CLASSES = N.FAILURE_MODES, N.PG_VAL_FAILURE_CLASSES
# the entries of failure_distribution: compute_failure_distribution's, minus the object properties
_DISTRIBUTION_KEYS = ("count", "frequency", "mean_episode_length", "std_episode_length", "mean_final_contacts",
                      "mean_confidence")
# columns of the robust row the validation keep-best may read (a plan with noise levels)
_VAL_ROBUST_SCORE_COLUMNS = ("worst_success_rate", "mean_success_rate", "mean_noisy_success_rate",
                             "worst_mean_return")


def column_index(name: Optional[str], what: str) -> int:
    if name is None:
        return -1
    if name not in _SCORE_COLUMNS:
        raise ValueError(f"{what} must be one of {list(_SCORE_COLUMNS)} or None, got {name!r}")
    return COLUMNS.index(name)


# ====================================================================== OptimizerLog
class OptimizerLog:
    """The step-size rows of a run on a trainer with step-size control: f64 [rows][8], one row per
    logged iteration (``column(name)`` / ``log.optimizer["lr"]``, names in OPT_COLUMNS): ``lr`` /
    ``lr_last`` the learning rate of the iteration's first / last applied pass (0: none applied),
    ``updates`` / ``skipped`` its passes applied / copied through, ``stop_pass`` the pass the KL
    stop hit (-1: none), ``kl_max`` the largest pass KL, ``kl_epoch`` the last epoch's KL over
    every sample, ``lr_scale`` the KL-adaptive scale the next iteration starts with."""

    def __init__(self, table):
        self.table = np.array(table, dtype=np.float64).reshape(-1, OPT_COLS)

    def column(self, name: str) -> np.ndarray:
        if name not in OPT_COLUMNS:
            raise ValueError(f"an optimizer column is one of {list(OPT_COLUMNS)}, got {name!r}")
        return self.table[:, OPT_COLUMNS.index(name)]

    __getitem__ = column

    @property
    def columns(self) -> Dict[str, np.ndarray]:
        return {name: self.table[:, k] for k, name in enumerate(OPT_COLUMNS)}

    def __len__(self) -> int:
        return self.table.shape[0]


# ====================================================================== ValueNormLog
class ValueNormLog:
    """The value-normalisation rows of a run on a trainer with popart: f64 [rows][14], one row per
    logged iteration, written by the iteration's dxrl_pg_popart_rescale launch (``column(name)`` /
    ``log.value_norm["sigma"]``, names in VNORM_COLUMNS).  ``mu`` / ``sigma``: the pair the next
    iteration decodes and encodes with -- ``sigma`` is the factor between the log's ``value_mse``
    (normalised units) and raw units, ``value_mse * sigma ** 2`` being the raw figure for targets
    encoded with that pair; ``mu_prev`` / ``sigma_prev``: the pair of the iteration itself;
    ``scale`` / ``shift`` / ``rescaled``: what the rescale did to the head; ``count`` / ``mean`` /
    ``std``: the running return moments; ``batch_mean`` / ``batch_std``: the iteration's own;
    ``calls``: batches folded; ``forget``: the forgetting factor.  A row of a refused rescale
    (``popart_state()["skipped"]``) stays zero."""

    def __init__(self, table):
        self.table = np.array(table, dtype=np.float64).reshape(-1, VNORM_COLS)

    def column(self, name: str) -> np.ndarray:
        if name not in VNORM_COLUMNS:
            raise ValueError(f"a value_norm column is one of {list(VNORM_COLUMNS)}, got {name!r}")
        return self.table[:, VNORM_COLUMNS.index(name)]

    __getitem__ = column

    @property
    def columns(self) -> Dict[str, np.ndarray]:
        return {name: self.table[:, k] for k, name in enumerate(VNORM_COLUMNS)}

    def __len__(self) -> int:
        return self.table.shape[0]


# ====================================================================== TrainingLog
class TrainingLog:
    """The learning curve of a run: one row per iteration, named NumPy columns
    (``log["mean_return"]``, ``log.columns``), the best and the convergence iteration.

    ``best_iteration``: the ``iteration`` value of the row keep-best chose (None: no row
    qualified).  ``convergence_iteration``: the ``iteration`` value of row
    ``converged_row - W + 1``, the first row of the first window whose mean exceeded the
    threshold (reward_comparison.py:121-124), or None.

    ``ranks``: f64 [rows][world][RANK_DOUBLES], the ranks' records every row was finished from
    (``rank_column(name)`` -> [rows][world], names in RANK_COLUMNS), for a run logged with
    ``fit(merge_ranks=True)``; None otherwise.

    ``optimizer``: the ``OptimizerLog`` of a run on a trainer with step-size control; None
    otherwise.  ``value_norm``: the ``ValueNormLog`` of a run on a trainer with popart; None
    otherwise."""

    def __init__(self, table=None, header: Optional[Dict[str, Any]] = None, window: Optional[int] = None,
                 settings: Optional[Dict[str, Any]] = None, _pending=None, validation: "Optional[ValidationLog]" = None,
                 ranks=None, optimizer=None, value_norm=None):
        self._pending = _pending
        self._optimizer = None if optimizer is None else OptimizerLog(optimizer)
        self._value_norm = None if value_norm is None else ValueNormLog(value_norm)
        self._ranks = None if ranks is None else np.array(ranks, dtype=np.float64)
        if self._ranks is not None and (self._ranks.ndim != 3 or self._ranks.shape[2] != RANK_DOUBLES):
            raise ValueError(f"ranks must be [rows][world][{RANK_DOUBLES}], got shape {self._ranks.shape}")
        self._table = None if table is None else np.array(table, dtype=np.float64).reshape(-1, COLS)
        self._header = dict(header) if header is not None else None
        self.window = window
        self.settings = dict(settings or {})
        self.validation = validation  # the held-out curve of fit(validation=plan), or None

    # -- lazy fill (fit enqueued the copy; the first read waits for it)
    def _resolve(self):
        if self._pending is not None:
            event, host_table, host_header, rows, host_ranks, host_opt, host_vnorm = self._pending
            event.synchronize()
            if host_opt is not None:
                self._optimizer = OptimizerLog(host_opt[:rows].numpy().copy())
            if host_vnorm is not None:
                self._value_norm = ValueNormLog(host_vnorm[:rows].numpy().copy())
            self._table = host_table[:rows].numpy().copy()
            self._header = header_dict(host_header.numpy())
            if host_ranks is not None:
                self._ranks = host_ranks[:rows].numpy().copy()
            self._pending = None

    @property
    def table(self) -> np.ndarray:
        self._resolve()
        return self._table

    @property
    def header(self) -> Dict[str, Any]:
        self._resolve()
        return self._header

    @property
    def ranks(self) -> Optional[np.ndarray]:
        """f64 [rows][world][RANK_DOUBLES], or None for a run logged without merge_ranks."""
        self._resolve()
        return self._ranks

    @property
    def optimizer(self) -> Optional[OptimizerLog]:
        """The step-size rows (OptimizerLog), or None for a trainer without step-size control."""
        self._resolve()
        return self._optimizer

    @property
    def value_norm(self) -> Optional[ValueNormLog]:
        """The value-normalisation rows (ValueNormLog), or None for a trainer without popart."""
        self._resolve()
        return self._value_norm

    def rank_column(self, name: str) -> np.ndarray:
        """[rows][world]: one entry of the ranks' records."""
        if self.ranks is None:
            raise ValueError("this log has no per-rank records (fit(..., merge_ranks=True))")
        if name not in RANK_COLUMNS:
            raise ValueError(f"a rank column is one of {list(RANK_COLUMNS)}, got {name!r}")
        return self.ranks[:, :, RANK_COLUMNS.index(name)]

    @property
    def columns(self) -> Dict[str, np.ndarray]:
        t = self.table
        return {name: t[:, k] for k, name in enumerate(COLUMNS)}

    def __getitem__(self, name: str) -> np.ndarray:
        return self.table[:, COLUMNS.index(name)]

    def __len__(self) -> int:
        return self.table.shape[0]

    @property
    def best_row(self) -> Optional[int]:
        r = int(self.header["best_row"])
        return r if r >= 0 else None

    @property
    def best_iteration(self) -> Optional[int]:
        r = self.best_row
        return None if r is None else int(self["iteration"][r])

    @property
    def converged_row(self) -> Optional[int]:
        r = int(self.header["converged_row"])
        return r if r >= 0 else None

    @property
    def convergence_iteration(self) -> Optional[int]:
        r = self.converged_row
        if r is None or not self.window:
            return None
        return int(self["iteration"][r - int(self.window) + 1])

    def statistics(self) -> Dict[str, Any]:
        """Scalars of the run (NaN-aware: rows without a finished episode carry NaN)."""
        n = len(self)
        out: Dict[str, Any] = {"iterations": n, "best_iteration": self.best_iteration,
                               "convergence_iteration": self.convergence_iteration,
                               "best_score": float(self.header["best_score"]) if self.best_row is not None else None}
        if n == 0:
            return out
        out["env_steps"] = int(self["env_steps"][-1])
        out["episodes"] = int(self["episodes"].sum())
        for name in ("mean_return", "success_rate", "mean_length", "explained_variance", "value_mse", "grad_norm"):
            col = self[name]
            ok = col[~np.isnan(col)]
            out[f"final_{name}"] = float(col[-1])
            out[f"average_{name}"] = float(ok.mean()) if ok.size else float("nan")
            out[f"max_{name}"] = float(ok.max()) if ok.size else float("nan")
        return out

    # -- JSON (NaN and the infinities as strings, so the file is standard JSON)
    def to_dict(self) -> Dict[str, Any]:
        out = {"format": LOG_FORMAT, "columns": list(COLUMNS), "window": self.window, "settings": self.settings,
               "header": {k: _enc(v) for k, v in self.header.items()},
               "rows": [[_enc(x) for x in row[:len(COLUMNS)]] for row in self.table.tolist()]}
        if self.validation is not None:  # a log without validation serialises as it always did
            out["validation"] = self.validation.to_dict()
        if self.ranks is not None:  # likewise: a run without merge_ranks serialises as it always did
            out["rank_columns"] = list(RANK_COLUMNS)
            out["ranks"] = [[[_enc(x) for x in rec] for rec in row] for row in self.ranks.tolist()]
        if self.optimizer is not None:  # likewise: a run without step-size control
            out["optimizer_columns"] = list(OPT_COLUMNS)
            out["optimizer"] = [[_enc(x) for x in row] for row in self.optimizer.table.tolist()]
        if self.value_norm is not None:  # likewise: a run without popart
            out["value_norm_columns"] = list(VNORM_COLUMNS)
            out["value_norm"] = [[_enc(x) for x in row] for row in self.value_norm.table.tolist()]
        return out

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "TrainingLog":
        if d.get("format") != LOG_FORMAT or list(d.get("columns", [])) != list(COLUMNS):
            raise ValueError(f"not a {LOG_FORMAT} log with this build's columns")
        table = np.zeros((len(d["rows"]), COLS), dtype=np.float64)
        for r, row in enumerate(d["rows"]):
            table[r, :len(COLUMNS)] = [_dec(x) for x in row]
        val = ValidationLog.from_dict(d["validation"]) if d.get("validation") is not None else None
        ranks = None
        if d.get("ranks") is not None:  # absent in runs without merge_ranks and in older files
            if list(d.get("rank_columns", [])) != list(RANK_COLUMNS):
                raise ValueError("not a training log with this build's rank columns")
            ranks = np.array([[[_dec(x) for x in rec] for rec in row] for row in d["ranks"]], dtype=np.float64)
            ranks = ranks.reshape(len(d["rows"]), -1, RANK_DOUBLES)
        opt = None
        if d.get("optimizer") is not None:  # absent in runs without step-size control and in older files
            if list(d.get("optimizer_columns", [])) != list(OPT_COLUMNS):
                raise ValueError("not a training log with this build's optimizer columns")
            opt = np.array([[_dec(x) for x in row] for row in d["optimizer"]], dtype=np.float64).reshape(-1, OPT_COLS)
        vn = None
        if d.get("value_norm") is not None:  # absent in runs without popart and in older files
            if list(d.get("value_norm_columns", [])) != list(VNORM_COLUMNS):
                raise ValueError("not a training log with this build's value_norm columns")
            vn = np.array([[_dec(x) for x in row] for row in d["value_norm"]], dtype=np.float64).reshape(-1, VNORM_COLS)
        return cls(table, {k: _dec(v) for k, v in d["header"].items()}, d.get("window"), d.get("settings"),
                   validation=val, ranks=ranks, optimizer=opt, value_norm=vn)

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, allow_nan=False)

    @classmethod
    def load(cls, path) -> "TrainingLog":
        with open(path) as f:
            return cls.from_dict(json.load(f))


def _enc(x):
    if isinstance(x, float) and not math.isfinite(x):
        return "nan" if math.isnan(x) else ("inf" if x > 0 else "-inf")
    return x


def _dec(x):
    return float(x) if isinstance(x, str) else x


def header_dict(raw: np.ndarray) -> Dict[str, Any]:
    """dxrl_pg_log_header bytes -> {rows_written, best_row, converged_row, best_score}."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    i, f = raw[:32].view(np.int64), raw[32:64].view(np.float64)
    return {"rows_written": int(i[0]), "best_row": int(i[1]), "converged_row": int(i[2]), "best_score": float(f[0])}


# ====================================================================== ValidationLog
class ValidationLog:
    """The held-out curve of a run: one row per validation (``log.validation["success_rate"]``,
    ``.columns``), the per-object success counts of every row with the objects' names, and the
    iteration keep-best chose / patience ran out at (None: none).

    A plan with noise levels adds ``noise_levels`` (the (obs_std, dyn_std) pairs, baseline first),
    ``levels`` (f64 [rows][L][12], ``level_column(name)`` -> [rows][L]), ``robust`` (f64 [rows][8],
    ``robust_column(name)``), ``level_results(row)``, and ``object_successes`` becomes
    [rows][L][objects]; the main table is then level 0, the clean curve.  Without levels these
    are None.

    A plan with common random numbers across the levels adds ``paired`` (f64 [rows][L][14],
    ``paired_column(name)`` -> [rows][L]: every level's episodes paired with the baseline's) and
    ``object_lost`` (i32 [rows][L][objects]: the lost pairs of each object).  Without it these are
    None.

    A plan with failure modes adds ``failure_modes`` (f64 [rows][L][6][10], ``failure_column(name)``
    -> [rows][L][6], modes in FAILURE_MODE_NAMES order), ``failure_levels`` (f64 [rows][L][8],
    ``failure_level_column(name)`` -> [rows][L]), ``failure_distribution(row, level)`` and -- with
    common random numbers -- ``failure_transitions`` (i32 [rows][L][7][7], ``transitions(row,
    level)``); L is 1 for a plan without noise levels.  Without the option these are None."""

    def __init__(self, table=None, header: Optional[Dict[str, Any]] = None, object_successes=None,
                 object_names=(), settings: Optional[Dict[str, Any]] = None, _pending=None, noise_levels=None,
                 levels=None, robust=None, paired=None, object_lost=None, failure_modes=None, failure_levels=None,
                 failure_transitions=None):
        self._pending = _pending
        self.object_names = list(object_names)
        self.noise_levels = None if noise_levels is None else [(float(o), float(d)) for o, d in noise_levels]
        L = self.num_levels
        self._table = None if table is None else np.array(table, dtype=np.float64).reshape(-1, VAL_COLS)
        self._header = dict(header) if header is not None else None
        shape = (-1, L, len(self.object_names)) if L else (-1, len(self.object_names))
        self._objects = None if object_successes is None else np.array(object_successes, dtype=np.int32).reshape(shape)
        self._levels = None if levels is None or not L else \
            np.array(levels, dtype=np.float64).reshape(-1, L, VAL_LEVEL_COLS)
        self._robust = None if robust is None or not L else \
            np.array(robust, dtype=np.float64).reshape(-1, VAL_ROBUST_COLS)
        self._paired = None if paired is None or not L else \
            np.array(paired, dtype=np.float64).reshape(-1, L, VAL_PAIRED_COLS)
        self._object_lost = None if object_lost is None or self._paired is None else \
            np.array(object_lost, dtype=np.int32).reshape(-1, L, len(self.object_names))
        Lf = max(L, 1)  # a validation without levels is one level
        self._failure_modes = None if failure_modes is None else \
            np.array(failure_modes, dtype=np.float64).reshape(-1, Lf, _MODES, VAL_FAILURE_MODE_COLS)
        self._failure_levels = None if failure_levels is None or self._failure_modes is None else \
            np.array(failure_levels, dtype=np.float64).reshape(-1, Lf, VAL_FAILURE_LEVEL_COLS)
        self._failure_transitions = None if failure_transitions is None or self._failure_modes is None else \
            np.array(failure_transitions, dtype=np.int32).reshape(-1, Lf, _CLASSES, _CLASSES)
        self.settings = dict(settings or {})

    @property
    def num_levels(self) -> int:
        return 0 if self.noise_levels is None else len(self.noise_levels)

    def _resolve(self):
        if self._pending is not None:
            event, host_table, host_header, host_objects, rows, more = self._pending
            event.synchronize()
            self._table = host_table[:rows].numpy().copy()
            self._header = val_header_dict(host_header.numpy())
            self._objects = host_objects[:rows].numpy().copy()
            for name, t in more.items():  # the optional tables of the plan, by _ValState's names
                setattr(self, "_" + name, t[:rows].numpy().copy())
            self._pending = None

    @property
    def table(self) -> np.ndarray:
        self._resolve()
        return self._table

    @property
    def header(self) -> Dict[str, Any]:
        self._resolve()
        return self._header

    @property
    def object_successes(self) -> np.ndarray:
        """i32 [rows][objects] ([rows][levels][objects] with noise levels): successes of each
        object (out of episodes / objects per row and level)."""
        self._resolve()
        return self._objects

    @property
    def levels(self) -> Optional[np.ndarray]:
        """f64 [rows][L][12] (VAL_LEVEL_COLUMNS), or None without noise levels."""
        self._resolve()
        return self._levels

    @property
    def robust(self) -> Optional[np.ndarray]:
        """f64 [rows][8] (VAL_ROBUST_COLUMNS), or None without noise levels."""
        self._resolve()
        return self._robust

    @property
    def paired(self) -> Optional[np.ndarray]:
        """f64 [rows][L][14] (VAL_PAIRED_COLUMNS), or None without common random numbers."""
        self._resolve()
        return self._paired

    @property
    def object_lost(self) -> Optional[np.ndarray]:
        """i32 [rows][L][objects]: per object, the episodes the baseline solved and the level did
        not; None without common random numbers."""
        self._resolve()
        return self._object_lost

    def paired_column(self, name: str) -> np.ndarray:
        """[rows][L]: one column of the paired rows."""
        if self.paired is None:
            raise ValueError("this validation has no paired table (validation_plan(..., noise_levels=..., "
                             "common_random_numbers=True))")
        return self.paired[:, :, VAL_PAIRED_COLUMNS.index(name)]

    @property
    def failure_modes(self) -> Optional[np.ndarray]:
        """f64 [rows][L][6][10] (FAILURE_MODE_NAMES x VAL_FAILURE_MODE_COLUMNS), or None without
        failure modes; L is 1 without noise levels."""
        self._resolve()
        return self._failure_modes

    @property
    def failure_levels(self) -> Optional[np.ndarray]:
        """f64 [rows][L][8] (VAL_FAILURE_LEVEL_COLUMNS), or None without failure modes."""
        self._resolve()
        return self._failure_levels

    @property
    def failure_transitions(self) -> Optional[np.ndarray]:
        """i32 [rows][L][7][7] ([from][to] over FAILURE_CLASS_NAMES: the baseline's class against
        the level's, per pair), or None without failure modes or without common random numbers."""
        self._resolve()
        return self._failure_transitions

    def _need_failure_modes(self):
        if self.failure_modes is None:
            raise ValueError("this validation has no failure tables (validation_plan(..., failure_modes=True))")

    def _failure_cell(self, row: int, level: int):
        self._need_failure_modes()
        rows, levels = self.failure_modes.shape[:2]
        if not -rows <= row < rows:
            raise IndexError(f"row {row} outside the {rows} validations of this log")
        if not 0 <= level < levels:
            raise IndexError(f"level {level} outside the {levels} levels of this validation")
        return row, level

    def failure_column(self, name: str) -> np.ndarray:
        """[rows][L][6]: one column of the mode rows."""
        self._need_failure_modes()
        if name not in VAL_FAILURE_MODE_COLUMNS:
            raise ValueError(f"a failure column is one of {list(VAL_FAILURE_MODE_COLUMNS)}, got {name!r}")
        return self.failure_modes[:, :, :, VAL_FAILURE_MODE_COLUMNS.index(name)]

    def failure_level_column(self, name: str) -> np.ndarray:
        """[rows][L]: one column of the per-level failure rows."""
        self._need_failure_modes()
        if name not in VAL_FAILURE_LEVEL_COLUMNS:
            raise ValueError(f"a failure level column is one of {list(VAL_FAILURE_LEVEL_COLUMNS)}, got {name!r}")
        return self.failure_levels[:, :, VAL_FAILURE_LEVEL_COLUMNS.index(name)]

    def failure_distribution(self, row: int, level: int = 0) -> Dict[str, Dict[str, Any]]:
        """The modes of one validation and level in ``compute_failure_distribution``'s shape (its
        entries minus the object properties), keyed by mode name, for the modes that occurred."""
        row, level = self._failure_cell(row, level)
        out = {}
        for m, name in enumerate(FAILURE_MODE_NAMES):
            r = self.failure_modes[row, level, m]
            if r[0] > 0:
                out[name] = {k: (int(r[0]) if k == "count" else float(r[VAL_FAILURE_MODE_COLUMNS.index(k)]))
                             for k in _DISTRIBUTION_KEYS}
        return out

    def transitions(self, row: int, level: int) -> Dict[str, Any]:
        """The class pairs of one validation and level: ``{"classes": FAILURE_CLASS_NAMES,
        "counts": i32 [7][7]}`` with counts[from][to] the pairs whose baseline episode has class
        ``from`` and whose episode in the level has class ``to``."""
        row, level = self._failure_cell(row, level)
        if self.failure_transitions is None:
            raise ValueError("this validation has no transitions (validation_plan(..., noise_levels=..., "
                             "common_random_numbers=True, failure_modes=True))")
        return {"classes": list(FAILURE_CLASS_NAMES), "counts": self.failure_transitions[row, level].copy()}

    def _need_levels(self):
        if not self.num_levels:
            raise ValueError("this validation has no noise levels (validation_plan(..., noise_levels=...))")

    def level_column(self, name: str) -> np.ndarray:
        """[rows][L]: one column of the level rows."""
        self._need_levels()
        return self.levels[:, :, VAL_LEVEL_COLUMNS.index(name)]

    def robust_column(self, name: str) -> np.ndarray:
        self._need_levels()
        return self.robust[:, VAL_ROBUST_COLUMNS.index(name)]

    @property
    def robust_columns(self) -> Dict[str, np.ndarray]:
        self._need_levels()
        return {name: self.robust[:, k] for k, name in enumerate(VAL_ROBUST_COLUMNS)}

    def level_results(self, row: int):
        """The levels of one validation as ``RobustnessTester`` result dictionaries, in its order:
        ``{"noise_levels": {observation_noise_std, dynamics_noise_std}, "metrics": {...}}``."""
        self._need_levels()
        out = []
        for (o, d), r in zip(self.noise_levels, self.levels[row]):
            out.append({"noise_levels": {"observation_noise_std": o, "dynamics_noise_std": d},
                        "metrics": {name: float(r[k]) for k, name in enumerate(VAL_LEVEL_COLUMNS) if k >= 2}})
        return out

    @property
    def columns(self) -> Dict[str, np.ndarray]:
        t = self.table
        return {name: t[:, k] for k, name in enumerate(VAL_COLUMNS)}

    def __getitem__(self, name: str) -> np.ndarray:
        return self.table[:, VAL_COLUMNS.index(name)]

    def __len__(self) -> int:
        return self.table.shape[0]

    def _row(self, key: str) -> Optional[int]:
        r = int(self.header[key])
        return r if r >= 0 else None

    @property
    def best_row(self) -> Optional[int]:
        return self._row("best_row")

    @property
    def best_iteration(self) -> Optional[int]:
        r = self.best_row
        return None if r is None else int(self["iteration"][r])

    @property
    def stopped_row(self) -> Optional[int]:
        return self._row("stopped_row")

    @property
    def stopped_iteration(self) -> Optional[int]:
        r = self.stopped_row
        return None if r is None else int(self["iteration"][r])

    def statistics(self) -> Dict[str, Any]:
        n = len(self)
        out: Dict[str, Any] = {"validations": n, "best_iteration": self.best_iteration,
                               "stopped_iteration": self.stopped_iteration,
                               "best_score": float(self.header["best_score"]) if self.best_row is not None else None}
        if n == 0:
            return out
        out["episodes_per_validation"] = int(self["episodes"][-1])
        for name in ("success_rate", "mean_return", "mean_length", "min_object_success_rate", "objects_solved"):
            col = self[name]
            out[f"final_{name}"] = float(col[-1])
            out[f"max_{name}"] = float(np.nanmax(col)) if not np.isnan(col).all() else float("nan")
        if self.num_levels:
            out["noise_levels"] = self.num_levels
            for name in ("worst_success_rate", "mean_success_rate", "max_degradation_percentage"):
                out[f"final_{name}"] = float(self.robust_column(name)[-1])
        if self.paired is not None:
            out["common_random_numbers"] = True
            if self.num_levels > 1:  # over the noisy levels of the last row
                out["final_max_lost"] = float(self.paired_column("lost")[-1, 1:].max())
                out["final_min_mean_return_diff"] = float(self.paired_column("mean_return_diff")[-1, 1:].min())
        if self.failure_modes is not None:  # per level of the last row (None: no failure in the level)
            dominant = self.failure_level_column("dominant_mode")[-1]
            out["final_dominant_failure_mode"] = [FAILURE_MODE_NAMES[int(m)] if m >= 0 else None for m in dominant]
            out["final_dominant_failure_frequency"] = [float(x) for x in
                                                       self.failure_level_column("dominant_frequency")[-1]]
            out["final_failure_rate"] = [float(x) for x in self.failure_level_column("failure_rate")[-1]]
        return out

    def to_dict(self) -> Dict[str, Any]:
        out = {"columns": list(VAL_COLUMNS), "settings": self.settings, "object_names": self.object_names,
               "header": {k: _enc(v) for k, v in self.header.items()},
               "rows": [[_enc(x) for x in row[:len(VAL_COLUMNS)]] for row in self.table.tolist()],
               "object_successes": self.object_successes.tolist()}
        if self.num_levels:  # a validation without levels serialises as it always did
            out["noise_levels"] = [list(p) for p in self.noise_levels]
            out["level_columns"], out["robust_columns"] = list(VAL_LEVEL_COLUMNS), list(VAL_ROBUST_COLUMNS)
            out["levels"] = [[[_enc(x) for x in lv] for lv in row] for row in self.levels.tolist()]
            out["robust"] = [[_enc(x) for x in row] for row in self.robust.tolist()]
        if self.paired is not None:  # a validation without common random numbers serialises as it always did
            out["paired_columns"] = list(VAL_PAIRED_COLUMNS)
            out["paired"] = [[[_enc(x) for x in lv] for lv in row] for row in self.paired.tolist()]
            out["object_lost"] = self.object_lost.tolist()
        if self.failure_modes is not None:  # a validation without failure modes serialises as it always did
            out["failure_mode_names"] = list(FAILURE_MODE_NAMES)
            out["failure_mode_columns"] = list(VAL_FAILURE_MODE_COLUMNS)
            out["failure_level_columns"] = list(VAL_FAILURE_LEVEL_COLUMNS)
            out["failure_modes"] = self.failure_modes.tolist()  # finite by construction
            out["failure_levels"] = self.failure_levels.tolist()
            if self.failure_transitions is not None:
                out["failure_transitions"] = self.failure_transitions.tolist()
        return out

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "ValidationLog":
        if list(d.get("columns", [])) != list(VAL_COLUMNS):
            raise ValueError("not a validation log with this build's columns")
        table = np.zeros((len(d["rows"]), VAL_COLS), dtype=np.float64)
        for r, row in enumerate(d["rows"]):
            table[r, :len(VAL_COLUMNS)] = [_dec(x) for x in row]
        noise = d.get("noise_levels")  # absent in logs without levels and in older files
        levels = robust = None
        if noise is not None:
            if list(d.get("level_columns", [])) != list(VAL_LEVEL_COLUMNS) or \
                    list(d.get("robust_columns", [])) != list(VAL_ROBUST_COLUMNS):
                raise ValueError("not a validation log with this build's level / robust columns")
            levels = np.array([[[_dec(x) for x in lv] for lv in row] for row in d["levels"]], dtype=np.float64)
            robust = np.array([[_dec(x) for x in row] for row in d["robust"]], dtype=np.float64)
        paired = object_lost = None
        if noise is not None and d.get("paired") is not None:  # absent without common random numbers
            if list(d.get("paired_columns", [])) != list(VAL_PAIRED_COLUMNS):
                raise ValueError("not a validation log with this build's paired columns")
            paired = np.array([[[_dec(x) for x in lv] for lv in row] for row in d["paired"]], dtype=np.float64)
            object_lost = d["object_lost"]
        failure = {}
        if d.get("failure_modes") is not None:  # absent without failure modes and in older files
            if list(d.get("failure_mode_names", [])) != list(FAILURE_MODE_NAMES) or \
                    list(d.get("failure_mode_columns", [])) != list(VAL_FAILURE_MODE_COLUMNS) or \
                    list(d.get("failure_level_columns", [])) != list(VAL_FAILURE_LEVEL_COLUMNS):
                raise ValueError("not a validation log with this build's failure modes and columns")
            failure = dict(failure_modes=d["failure_modes"], failure_levels=d["failure_levels"],
                           failure_transitions=d.get("failure_transitions"))
        return cls(table, {k: _dec(v) for k, v in d["header"].items()}, d["object_successes"], d["object_names"],
                   d.get("settings"), noise_levels=noise, levels=levels, robust=robust, paired=paired,
                   object_lost=object_lost, **failure)


def val_header_dict(raw: np.ndarray) -> Dict[str, Any]:
    """dxrl_pg_val_header bytes -> {rows_written, best_row, stopped_row, since_best, best_score}."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    i, f = raw[:32].view(np.int64), raw[32:64].view(np.float64)
    return {"rows_written": int(i[0]), "best_row": int(i[1]), "stopped_row": int(i[2]), "since_best": int(i[3]),
            "best_score": float(f[0])}


def val_column_index(name: Optional[str], what: str = "val_keep_best") -> int:
    if name is None:
        return -1
    if name not in _VAL_SCORE_COLUMNS:
        raise ValueError(f"{what} must be one of {list(_VAL_SCORE_COLUMNS)} or None, got {name!r}")
    return VAL_COLUMNS.index(name)


def val_score(name: Optional[str], has_levels: bool, what: str = "val_keep_best"):
    """(score_table, score_col) of a validation keep-best column: a column of the main row
    (table 0), or -- for a plan with noise levels -- one of the robust row's score columns
    (table 1)."""
    if name in _VAL_ROBUST_SCORE_COLUMNS:
        if not has_levels:
            raise ValueError(f"{what}={name!r} is a score over noise levels: it needs a validation plan built "
                             "with noise_levels")
        return 1, VAL_ROBUST_COLUMNS.index(name)
    if name is not None and name not in _VAL_SCORE_COLUMNS:
        raise ValueError(f"{what} must be one of {list(_VAL_SCORE_COLUMNS)}, (with noise levels) "
                         f"{list(_VAL_ROBUST_SCORE_COLUMNS)} or None, got {name!r}")
    return 0, val_column_index(name, what)


def parse_noise_levels(noise_levels):
    """The (obs_std, dyn_std) pairs of a levels plan as a list of float pairs with the baseline
    (0.0, 0.0) first (inserted when absent; moved to the front when given later).  ValueError for a
    level that is not a pair of finite values >= 0, a duplicate, or more than
    N.PG_VAL_MAX_LEVELS levels."""
    levels = []
    for lv in noise_levels:
        try:
            o, d = (float(x) for x in lv)
        except (TypeError, ValueError):
            raise ValueError(f"a noise level is an (obs_std, dyn_std) pair, got {lv!r}") from None
        if not (math.isfinite(o) and math.isfinite(d)) or o < 0.0 or d < 0.0:
            raise ValueError(f"noise standard deviations must be finite and >= 0, got {lv!r}")
        if (o, d) in levels:
            raise ValueError(f"duplicate noise level {(o, d)!r}")
        levels.append((o, d))
    if (0.0, 0.0) in levels:
        levels.remove((0.0, 0.0))
    levels.insert(0, (0.0, 0.0))
    if len(levels) > N.PG_VAL_MAX_LEVELS:
        raise ValueError(f"{len(levels)} noise levels (with the baseline): at most {N.PG_VAL_MAX_LEVELS}")
    return levels


# ====================================================================== validation plan
class ValidationPlan:
    """A held-out evaluation of the trainer's live actor, built once: what
    ``Evaluator.evaluate_heldout_set(K, seed, parallel=True, device_seed=device_seed)`` would
    launch (object-major records, one lane per episode, device Philox resets), with its env, lane
    and segment tables, record buffers, work-queue counter and status word kept for the plan's
    life.  ``run`` enqueues ``dxrl_evaluate_mlp`` on the trainer's packed weights and
    ``dxrl_pg_val_row`` behind it and reads nothing back.  Every run uses the same seeds (common
    random numbers across iterations), so rows are comparable across iterations.  The plan touches
    neither the training env nor the trainer's streams or buffers.

    ``noise_levels`` (a sequence of (obs_std, dyn_std) pairs; ``parse_noise_levels``) makes it a
    robustness sweep of the live actor: one lane per episode of every level, level-major (level
    l, object o, episode k is lane, segment and record (l G + o) K + k), each lane the segment
    ``Segment(o, [seed + k], obs_std, dyn_std)`` with device Philox noise, and
    ``dxrl_pg_val_levels_row`` behind the one episode launch.  Level 0 is the baseline and holds
    records 0 .. G K - 1, which are the plan without levels' records.  The device streams are keyed
    by lane, segment and record index, so by default the levels do not share spawns or noise draws
    and a degradation is the difference of two independent samples.

    ``common_random_numbers=True`` (needs ``noise_levels``) makes the random numbers common across
    the levels too: the episode launch runs with ``stream_period = G K``, so level l's episode i
    has the spawn, the object properties, the standard normals (scaled by the level's stds) and
    the action noise of the baseline's episode i.  Level 0 keeps its records; every level is what
    a plan of that level alone would run.  ``dxrl_pg_val_paired_row`` then adds the paired table
    (``ValidationLog.paired`` / ``.object_lost``) behind the levels row.

    ``failure_modes=True`` (with or without levels and common random numbers) makes the episode
    launch accumulate ``hist_moments`` and enqueues ``dxrl_pg_val_failure_row`` last: every episode
    is classified with the failure taxonomy (timeout bound ``classify_max_steps``, default the
    plan's ``max_steps``; ``success_threshold`` as ``FailureClassifier``'s) into
    ``ValidationLog.failure_modes`` / ``.failure_levels`` and, with common random numbers,
    ``.failure_transitions``.  The records and every other table keep their bytes."""

    def __init__(self, tr, heldout_set, episodes_per_object: int = 5, seed: int = 0, device_seed: int = 0,
                 max_steps: Optional[int] = None, deterministic: bool = True, solve_threshold: float = 1.0,
                 noise_levels=None, common_random_numbers: bool = False, failure_modes: bool = False,
                 classify_max_steps: Optional[int] = None, success_threshold: int = 3):
        from .envs import VecEnv
        from .evaluator import Evaluator, Segment
        objs = list(heldout_set.heldout_objects)
        G, K = len(objs), int(episodes_per_object)
        if G < 1 or K < 1:
            raise ValueError("a validation needs at least one held-out object and one episode per object")
        if G > N.MAX_CURRICULA:
            raise ValueError(f"{G} held-out objects: the env's curriculum table holds {N.MAX_CURRICULA} rows, one "
                             f"per object -- validate on at most {N.MAX_CURRICULA} objects")
        if seed is None:
            raise ValueError("a validation repeats the same episodes every time: seed must be an integer")
        self.noise_levels = None if noise_levels is None else parse_noise_levels(noise_levels)
        L = self.L = 0 if self.noise_levels is None else len(self.noise_levels)
        self.common_random_numbers = bool(common_random_numbers)
        if self.common_random_numbers and not L:
            raise ValueError("common_random_numbers pairs the episodes of the noise levels: it needs noise_levels")
        ms = int(max_steps or tr.env.max_episode_steps)
        self.failure_modes = bool(failure_modes)
        self.classify_max_steps = int(ms if classify_max_steps is None else classify_max_steps)
        self.success_threshold = int(success_threshold)
        if self.failure_modes:
            if ms > N.SUMMARY_MAX_STEPS:
                raise ValueError(f"failure_modes needs max_steps <= {N.SUMMARY_MAX_STEPS} (the exact integer "
                                 f"variance rule of the taxonomy), got {ms}")
            if G * K > N.PG_VAL_FAILURE_MAX_EPISODES:
                raise ValueError(f"failure_modes needs objects x episodes_per_object <= "
                                 f"{N.PG_VAL_FAILURE_MAX_EPISODES} (the exact integer variance of the lengths), "
                                 f"got {G * K}")
            if self.classify_max_steps < 1:
                raise ValueError(f"classify_max_steps must be >= 1, got {self.classify_max_steps}")
        dev = self.dev = tr.dev
        self.G, self.K, self.E, self.max_steps = G, K, max(L, 1) * G * K, ms
        if self.E > 2**31 - 1:
            raise ValueError(f"{self.E} validation episodes: levels x objects x episodes must fit 32 bits")
        self.seed, self.device_seed = int(seed), int(device_seed)
        self.deterministic, self.solve_threshold = bool(deterministic), float(solve_threshold)
        self.object_names = [f"object_{o}" for o in range(G)]
        ev = Evaluator(None, heldout_set, reward_type=tr.env.reward_type, max_episode_steps=ms, device=dev)
        program = ev.heldout_program(K, self.seed, parallel=True)
        if L:  # heldout_program's lanes (Segment(o, [seed + k])) once per level, with the level's noise
            program = ev._program(program.configs)
            for obs, dyn in self.noise_levels:
                for o in range(G):
                    for k in range(K):
                        program.add_lane([Segment(o, [self.seed + k], obs, dyn, noise_seed=(self.seed, k))])
        plan =program.plan(host_resets=False, host_noise=False)
        self.fingerprint = {"objects": [_config_state(c) for c in program.configs], "episodes_per_object": K,
                            "seed": self.seed, "device_seed": self.device_seed, "max_steps": ms,
                            "deterministic": self.deterministic, "solve_threshold": self.solve_threshold,
                            "reward_type": tr.env.reward_type}
        if L:  # a plan without levels keeps the fingerprint it always had
            self.fingerprint["noise_levels"] = [list(p) for p in self.noise_levels]
        if self.common_random_numbers:  # only when set: every other plan keeps its fingerprint
            self.fingerprint["common_random_numbers"] = True
        if self.failure_modes:  # likewise
            self.fingerprint["failure_modes"] = {"classify_max_steps": self.classify_max_steps,
                                                 "success_threshold": self.success_threshold}
        self.fingerprint = json.loads(json.dumps(self.fingerprint))  # as a checkpoint returns it
        E = self.E
        self.env = VecEnv(E, reward_type=tr.env.reward_type, reward_shaping=tr.env.reward_shaping,
                          max_episode_steps=ms, seed=self.device_seed, device=dev)
        self.env.set_curricula(program.configs)
        self.lane_off = torch.from_numpy(np.ascontiguousarray(plan.lane_off)).to(dev, torch.int32)
        self.segments = torch.from_numpy(plan.segments.view(np.uint8).copy()).to(dev)
        self.ep_return = torch.zeros(E, dtype=torch.float64, device=dev)
        self.ep_length = torch.zeros(E, dtype=torch.int32, device=dev)
        self.ep_success = torch.zeros(E, dtype=torch.uint8, device=dev)
        self.ep_contacts = torch.zeros(E, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.queue = torch.zeros(1, dtype=torch.int32, device=dev)
        nb = C.c_int64()
        if L:
            N.call("dxrl_pg_val_levels_partial_doubles", L, G, K, C.byref(nb))
            self.level_noise = torch.tensor(self.noise_levels, dtype=torch.float64, device=dev)
        else:
            N.call("dxrl_pg_val_partial_doubles", G, K, C.byref(nb))
        self.partial = torch.zeros(nb.value, dtype=torch.float64, device=dev)
        self.paired_partial = None
        if self.common_random_numbers:
            N.call("dxrl_pg_val_paired_partial_doubles", L, G, K, C.byref(nb))
            self.paired_partial = torch.zeros(nb.value, dtype=torch.float64, device=dev)
        self.hist_moments = self.failure_partial = None
        if self.failure_modes:
            self.hist_moments = torch.zeros(E, 5, dtype=torch.int32, device=dev)
            N.call("dxrl_pg_val_failure_partial_doubles", max(L, 1), G, K, C.byref(nb))
            self.failure_partial = torch.zeros(nb.value, dtype=torch.float64, device=dev)
        self.action_std = None  # exp(log_std) of the last stochastic run (kept alive for its launch)
        a = self.args = N.EvalArgs()
        a.num_lanes, a.policy, a.max_steps, a.total_episodes = E, N.EVAL_POLICY_MLP, ms, E
        a.lane_segments, a.segments = N.ptr(self.lane_off), N.ptr(self.segments)
        a.policy_seed = a.noise_seed = a.reset_seed = self.device_seed & (2**64 - 1)
        a.ep_return, a.ep_length, a.ep_success = N.ptr(self.ep_return), N.ptr(self.ep_length), N.ptr(self.ep_success)
        a.ep_contacts, a.status, a.work_queue = N.ptr(self.ep_contacts), N.ptr(self.status), N.ptr(self.queue)
        a.stream_period = G * K if self.common_random_numbers else 0
        a.hist_moments = N.ptr(self.hist_moments)  # NULL without failure modes: the launch it always was

    @staticmethod
    def sweep_levels(observation_noise_levels, dynamics_noise_levels):
        """The distinct (obs_std, dyn_std) levels of ``RobustnessTester.sweep_levels``, in its
        order.  With a 0.0 among the first three values of a list the reference's combined block
        repeats single-noise levels; a plan runs each level once, so a repeat is dropped."""
        from .evaluator import RobustnessTester
        obs, dyn = [float(x) for x in observation_noise_levels], [float(x) for x in dynamics_noise_levels]
        if not all(math.isfinite(x) and x >= 0.0 for x in obs + dyn):  # the sweep would skip them silently
            raise ValueError(f"noise standard deviations must be finite and >= 0, got {obs} and {dyn}")
        levels = RobustnessTester.sweep_levels(obs, dyn)[0]
        return list(dict.fromkeys((float(o), float(d)) for o, d in levels))

    def run(self, tr, val: "_ValState", iteration: int, env_steps: int, train_row: int, score_col: int = -1,
            min_delta: float = 0.0, patience: int = 0, score_table: int = 0):
        """Enqueue one validation of the trainer's current weights as row ``val.rows`` (no sync).
        ``tr.params`` is swapped with a spare buffer by every optimiser step, so the pointers are
        taken here.  ``score_table`` 1 (a plan with levels) reads the score from the robust row."""
        from .trainer import ACT, OFF
        if val.fingerprint != self.fingerprint:
            raise ValueError("this run's validation table was written by another plan (differs in "
                             f"{', '.join(fingerprint_diff(val.fingerprint, self.fingerprint))})")
        if score_table and not self.L:
            raise ValueError("a robust score needs a plan with noise levels")
        val.reserve(val.rows + 1)
        p = N.ptr
        with torch.cuda.device(self.dev):
            self.status.zero_()  # the episode kernel only ever sets bits of it
            m = N.EvalMlp()
            m.packed, m.params, m.action_std = p(tr.packed), p(tr.params), None
            if not self.deterministic:
                # f64 exp rounded to f32 (the kernel evaluates no exp)
                ls = tr.params[OFF["logstd"]:OFF["logstd"] + ACT]
                self.action_std = torch.exp(ls.double()).float()
                m.action_std = p(self.action_std)
            N.call("dxrl_evaluate_mlp", self.env.handle, C.byref(self.args), C.byref(m), tr._s())
            v = N.PgValLevelsArgs() if self.L else N.PgValArgs()
            v.num_objects, v.episodes_per_object, v.row, v.cap = self.G, self.K, val.rows, val.cap
            v.iteration, v.env_steps, v.train_row = int(iteration), int(env_steps), int(train_row)
            v.num_params, v.partial_doubles = tr.params.numel(), self.partial.numel()
            v.score_col, v.patience = int(score_col), int(patience)
            v.min_delta, v.solve_threshold = float(min_delta), self.solve_threshold
            v.ep_return, v.ep_length, v.ep_success = p(self.ep_return), p(self.ep_length), p(self.ep_success)
            v.ep_contacts, v.status = p(self.ep_contacts), p(self.status)
            v.params, v.best_params, v.partial = p(tr.params), p(val.best_params), p(self.partial)
            v.val, v.object_successes, v.header = p(val.table), p(val.objects), p(val.header)
            if self.L:
                v.num_levels, v.score_table, v.level_noise = self.L, int(score_table), p(self.level_noise)
                v.levels, v.robust = p(val.levels), p(val.robust)
                N.call("dxrl_pg_val_levels_row", self.dev.index, C.byref(v), tr._s())
                if self.common_random_numbers:
                    q = N.PgValPairedArgs()
                    q.num_objects, q.episodes_per_object, q.row, q.cap = self.G, self.K, val.rows, val.cap
                    q.num_levels, q.partial_doubles = self.L, self.paired_partial.numel()
                    q.ep_return, q.ep_length, q.ep_success = v.ep_return, v.ep_length, v.ep_success
                    q.partial, q.paired, q.object_lost = p(self.paired_partial), p(val.paired), p(val.object_lost)
                    N.call("dxrl_pg_val_paired_row", self.dev.index, C.byref(q), tr._s())
            else:
                N.call("dxrl_pg_val_row", self.dev.index, C.byref(v), tr._s())
            if self.failure_modes:  # last: behind the rows above, on records they only read
                q = N.PgValFailureArgs()
                q.num_objects, q.episodes_per_object, q.row, q.cap = self.G, self.K, val.rows, val.cap
                q.num_levels, q.paired = max(self.L, 1), int(self.common_random_numbers)
                q.partial_doubles = self.failure_partial.numel()
                q.max_steps, q.timeout_steps = self.max_steps, self.classify_max_steps
                q.success_threshold = self.success_threshold
                q.ep_length, q.ep_success, q.ep_contacts = v.ep_length, v.ep_success, v.ep_contacts
                q.hist_moments, q.partial = p(self.hist_moments), p(self.failure_partial)
                q.failure_modes, q.failure_levels = p(val.failure_modes), p(val.failure_levels)
                q.failure_transitions = p(val.failure_transitions)
                N.call("dxrl_pg_val_failure_row", self.dev.index, C.byref(q), tr._s())
        val.rows += 1


def fingerprint_diff(a: Dict[str, Any], b: Dict[str, Any]):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


class _ValState:
    """The device validation table, per-object table, header and validation-best parameters of a
    trainer's run (a second, independent set beside the training log's).  For a plan with noise
    levels (the fingerprint's noise_levels) also the level and robust tables, and the per-object
    table holds a row per level; with common random numbers (the fingerprint's
    common_random_numbers) also the paired table and the per-object lost pairs; with failure modes
    (the fingerprint's failure_modes) also the mode and level failure tables and, with common
    random numbers, the transitions."""

    def __init__(self, tr, fingerprint: Dict[str, Any], object_names, cap: int = 0):
        d = self.dev = tr.dev
        self.fingerprint, self.object_names, self.G = fingerprint, list(object_names), len(object_names)
        noise = fingerprint.get("noise_levels")
        self.noise_levels = None if noise is None else [(float(o), float(dd)) for o, dd in noise]
        self.L = 0 if noise is None else len(noise)
        self.crn = bool(self.L and fingerprint.get("common_random_numbers"))
        self.failures = fingerprint.get("failure_modes") is not None
        self.cap = 0
        self.table = self.objects = self.host_table = self.host_objects = None
        self.levels = self.robust = self.host_levels = self.host_robust = None
        self.paired = self.object_lost = self.host_paired = self.host_object_lost = None
        self.failure_modes = self.failure_levels = self.failure_transitions = None
        self.header = torch.zeros(_VAL_HEADER_BYTES, dtype=torch.uint8, device=d)
        self.header[8:24].view(torch.int64).fill_(-1)                  # best_row, stopped_row
        self.header[32:40].view(torch.float64).fill_(-math.inf)        # best_score
        self.host_header = torch.zeros(_VAL_HEADER_BYTES, dtype=torch.uint8).pin_memory()
        self.best_params = torch.zeros_like(tr.params)
        self.rows = 0
        self.settings: Dict[str, Any] = {}
        self.event = torch.cuda.Event()
        self.last_log = None
        self.reserve(cap)

    def _shapes(self, cap: int):
        """name -> (shape, dtype) of the run's validation tables."""
        shapes = {"table": ((cap, VAL_COLS), torch.float64),
                  "objects": ((cap, self.L, self.G) if self.L else (cap, self.G), torch.int32)}
        if self.L:
            shapes["levels"] = ((cap, self.L, VAL_LEVEL_COLS), torch.float64)
            shapes["robust"] = ((cap, VAL_ROBUST_COLS), torch.float64)
        if self.crn:
            shapes["paired"] = ((cap, self.L, VAL_PAIRED_COLS), torch.float64)
            shapes["object_lost"] = ((cap, self.L, self.G), torch.int32)
        if self.failures:
            Lf = max(self.L, 1)
            shapes["failure_modes"] = ((cap, Lf, _MODES, VAL_FAILURE_MODE_COLS), torch.float64)
            shapes["failure_levels"] = ((cap, Lf, VAL_FAILURE_LEVEL_COLS), torch.float64)
            if self.crn:
                shapes["failure_transitions"] = ((cap, Lf, _CLASSES, _CLASSES), torch.int32)
        return shapes

    def optional_tables(self):
        """The names of the plan's tables beyond the main one and the per-object one."""
        return [name for name in self._shapes(1) if name not in ("table", "objects")]

    def reserve(self, cap: int):
        if self.table is not None and cap <= self.cap:
            return
        cap = max(cap, _MIN_VAL_CAP, 2 * self.cap)
        for name, (shape, dtype) in self._shapes(cap).items():
            new, old = torch.zeros(shape, dtype=dtype, device=self.dev), getattr(self, name)
            if old is not None and self.rows:
                new[:self.rows].copy_(old[:self.rows])
            setattr(self, name, new)
            setattr(self, "host_" + name, torch.zeros(shape, dtype=dtype).pin_memory())
        self.cap = cap


def val_state(tr, st: "_RunState", plan: ValidationPlan) -> _ValState:
    """The run's validation state for `plan`: created on first use; a run validated by another
    plan (an earlier fit, or a checkpoint) raises."""
    if st.val is None:
        st.val = _ValState(tr, plan.fingerprint, plan.object_names)
    elif st.val.fingerprint != plan.fingerprint:
        raise ValueError("this run is validated by another plan (differs in "
                         f"{', '.join(fingerprint_diff(st.val.fingerprint, plan.fingerprint))}): a validation "
                         "table holds rows of one held-out set, episode count, seeds, step limit, mode, "
                         "noise levels, common-random-numbers and failure-modes setting")
    return st.val


def validation_log(tr) -> Optional[ValidationLog]:
    """The run's validation curve so far (None: never validated), filled like ``training_log``."""
    st = getattr(tr, "_run", None)
    v = st.val if st is not None else None
    if v is None:
        return None
    last = v.last_log() if v.last_log is not None else None
    if last is not None:
        last._resolve()
    optional = v.optional_tables()
    if v.rows:
        for name in ["table", "objects"] + optional:
            getattr(v, "host_" + name)[:v.rows].copy_(getattr(v, name)[:v.rows], non_blocking=True)
    v.host_header.copy_(v.header, non_blocking=True)
    v.event.record(torch.cuda.current_stream(tr.dev))
    more = {name: getattr(v, "host_" + name) for name in optional}
    log = ValidationLog(object_names=v.object_names, settings=v.settings, noise_levels=v.noise_levels,
                        _pending=(v.event, v.host_table, v.host_header, v.host_objects, v.rows, more))
    v.last_log = weakref.ref(log)
    return log


# ====================================================================== device state of a run
class _RunState:
    """The device table, header, best parameters and scratch of a trainer's run."""

    def __init__(self, tr, cap: int):
        d = tr.dev
        self.cap = 0
        self.table = None
        self.host_table = None
        self.header = torch.zeros(_HEADER_BYTES, dtype=torch.uint8, device=d)
        self.header[8:24].view(torch.int64).fill_(-1)                  # best_row, converged_row
        self.header[32:40].view(torch.float64).fill_(-math.inf)        # best_score
        self.host_header = torch.zeros(_HEADER_BYTES, dtype=torch.uint8).pin_memory()
        self.best_params = torch.zeros_like(tr.params)
        nb = C.c_int64()
        N.call("dxrl_pg_log_partial_doubles", tr.n, tr.T, C.byref(nb))
        self.partial = torch.zeros(nb.value, dtype=torch.float64, device=d)
        self.rows = 0
        self.env_steps = 0
        self.window: Optional[int] = None
        self.settings: Dict[str, Any] = {}
        self.host_reads = 0   # host reads of device memory made inside fit (polls)
        self.event = torch.cuda.Event()
        self.last_log = None  # weak reference to the last TrainingLog handed out
        self.val: Optional[_ValState] = None  # the validation tables (fit(validation=plan))
        # fit(merge_ranks=True): this rank's record, the gathered records and the per-rank log
        self.merged = False
        self.record = self.records_all = self.rank_log = self.host_rank_log = None
        # a trainer with step-size control: the optimizer table, one row per logged iteration
        self.controlled = bool(getattr(tr, "lr_control", False))
        self.opt_table = self.host_opt_table = None
        # a trainer with popart: the value_norm table, one row per logged iteration
        self.popart = getattr(tr, "popart", None) is not None
        self.vnorm_table = self.host_vnorm_table = None
        self.reserve(tr, cap)

    def merge_ranks(self, tr):
        """Make this run a rank-merged one (before its first row)."""
        if self.merged:
            return
        self.merged = True
        self.record = torch.zeros(RANK_DOUBLES, dtype=torch.float64, device=tr.dev)
        self.records_all = torch.zeros(tr.world, RANK_DOUBLES, dtype=torch.float64, device=tr.dev)
        self._rank_tables(tr, self.cap)

    def _rank_tables(self, tr, cap: int):
        rank_log = torch.zeros(cap, tr.world, RANK_DOUBLES, dtype=torch.float64, device=tr.dev)
        if self.rank_log is not None and self.rows:
            rank_log[:self.rows].copy_(self.rank_log[:self.rows])
        self.rank_log = rank_log
        self.host_rank_log = torch.zeros(cap, tr.world, RANK_DOUBLES, dtype=torch.float64).pin_memory()

    def reserve(self, tr, cap: int):
        """Room for `cap` rows: the table is allocated once per run and only regrown (device
        copy, no host sync) when a later fit needs more rows than it holds."""
        if self.table is not None and cap <= self.cap:
            return
        cap = max(cap, _MIN_CAP, 2 * self.cap)
        table = torch.zeros(cap, COLS, dtype=torch.float64, device=tr.dev)
        if self.table is not None and self.rows:
            table[:self.rows].copy_(self.table[:self.rows])
        self.table, self.cap = table, cap
        self.host_table = torch.zeros(cap, COLS, dtype=torch.float64).pin_memory()
        if self.controlled:
            opt = torch.zeros(cap, OPT_COLS, dtype=torch.float64, device=tr.dev)
            if self.opt_table is not None and self.rows:
                opt[:self.rows].copy_(self.opt_table[:self.rows])
            self.opt_table = opt
            self.host_opt_table = torch.zeros(cap, OPT_COLS, dtype=torch.float64).pin_memory()
        if self.popart:
            vn = torch.zeros(cap, VNORM_COLS, dtype=torch.float64, device=tr.dev)
            if self.vnorm_table is not None and self.rows:
                vn[:self.rows].copy_(self.vnorm_table[:self.rows])
            self.vnorm_table = vn
            self.host_vnorm_table = torch.zeros(cap, VNORM_COLS, dtype=torch.float64).pin_memory()
        if self.merged:
            self._rank_tables(tr, cap)


def run_state(tr, cap: int = 0) -> _RunState:
    st = getattr(tr, "_run", None)
    if st is None:
        st = tr._run = _RunState(tr, cap)
    else:
        st.reserve(tr, cap)
    return st


def log_iteration(tr, st: _RunState, score_col: int, min_episodes: int, conv_col: int, window: int,
                  threshold: float, merge_ranks: bool = False):
    """One dxrl_pg_log_row call for the iteration that just ran (enqueued, no sync).  With
    merge_ranks: dxrl_pg_log_rank_pack, one all-gather of the ranks' records on the compute
    stream, and dxrl_pg_log_row_world on the gathered records."""
    p = N.ptr
    a = N.PgLogArgs()
    a.num_envs, a.horizon, a.row, a.cap = tr.n, tr.T, st.rows, st.cap
    st.env_steps += tr.global_M if merge_ranks else tr.M
    a.iteration, a.env_steps = tr.iteration_index - 1, st.env_steps
    loss = tr.fused_loss if tr.cfg.fused else tr.loss_partial
    a.loss_blocks, a.loss_rows = loss.shape[0], (tr._loss_rows if tr.cfg.fused else tr.M)
    a.min_episodes, a.num_params, a.partial_doubles = int(min_episodes), tr.params.numel(), st.partial.numel()
    a.score_col, a.conv_col, a.conv_window, a.conv_threshold = score_col, conv_col, int(window), float(threshold)
    a.ep_count, a.ep_sum_return, a.ep_sum_length = p(tr.ep_count), p(tr.ep_sum_ret), p(tr.ep_sum_len)
    a.ep_successes, a.rew, a.ret, a.done, a.values = p(tr.ep_succ), p(tr.rew), p(tr.ret), p(tr.done), p(tr.values_raw)
    a.stats, a.loss_partial, a.gnorm2 = p(tr.stats), p(loss), p(tr.gnorm2)
    a.params, a.best_params = p(tr.params), p(st.best_params)
    a.partial, a.log, a.header = p(st.partial), p(st.table), p(st.header)
    if merge_ranks:
        from .distributed import all_gather_into_
        with torch.cuda.device(tr.dev):
            N.call("dxrl_pg_log_rank_pack", tr.dev.index, C.byref(a), p(st.record), tr._s())
            all_gather_into_(st.records_all, st.record, tr.world, tr.pg if tr.collective else None)
            N.call("dxrl_pg_log_row_world", tr.dev.index, C.byref(a), p(st.records_all), tr.world, p(st.rank_log),
                   tr._s())
    else:
        N.call("dxrl_pg_log_row", tr.dev.index, C.byref(a), tr._s())
    st.rows += 1


def fit(tr, iterations: int, keep_best: Optional[str] = "mean_return", min_episodes: int = 1, converge=None,
        stop_on_converge: bool = False, poll_every: int = 0, validation: Optional[ValidationPlan] = None,
        validate_every: int = 1, val_keep_best: Optional[str] = "success_rate", min_delta: float = 0.0,
        patience: int = 0, stop_on_patience: bool = False, merge_ranks: bool = False) -> TrainingLog:
    """Run `iterations` training iterations, logging each on the device.

    keep_best: the score column ("mean_return", "success_rate", any column before is_best, or
    None); a row is best iff it finished >= min_episodes episodes and its score is strictly above
    every earlier best.  converge: (column, window, threshold) -- converged at the first row
    whose window mean is strictly above the threshold.  With poll_every = k and
    stop_on_converge the header is read every k iterations and the run stops at the first poll
    after convergence; with poll_every = 0 the host reads nothing until the log is first used.
    A second fit on the same trainer continues the same log.

    validation: a ``ValidationPlan`` (``tr.validation_plan(heldout_set, ...)``).  After every
    validate_every-th logged iteration of the run, and after the last one of this call, the plan
    runs against the weights the next rollout would use and ``dxrl_pg_val_row`` appends a row to
    the run's validation table (``log.validation``): a second keep-best (val_keep_best, a column
    of the validation table; strictly above the best so far + min_delta) with its own best
    parameters (``tr.best_policy(which="validation")``), and patience: the validation header's
    stopped_row is the first row that is the patience-th in a row without a new best.  With
    stop_on_patience the validation header is read at the same polls, and the run stops at the
    first poll after stopped_row is set.  keep_best / converge on the training log are untouched.

    With a plan built with noise_levels every validation is a robustness sweep of the live actor
    (``dxrl_pg_val_levels_row``): ``log.validation`` keeps its columns as the clean (level 0)
    curve and gains ``levels`` / ``robust``, and val_keep_best may also name a score over the
    levels -- "worst_success_rate", "mean_success_rate", "mean_noisy_success_rate" or
    "worst_mean_return" -- which min_delta, patience and stop_on_patience then follow.  A plan
    built with common_random_numbers=True also logs ``paired`` / ``object_lost``
    (``dxrl_pg_val_paired_row``); keep-best and patience do not read them.  A plan built with
    failure_modes=True also logs ``failure_modes`` / ``failure_levels`` / ``failure_transitions``
    (``dxrl_pg_val_failure_row``); keep-best and patience do not read those either.

    merge_ranks: the run of a sharded (collective) trainer.  Every rank reduces its own tape to a
    record (``dxrl_pg_log_rank_pack``), the records are all-gathered -- one collective per logged
    iteration, on the compute stream -- and every rank finishes the row from the same gathered
    bytes (``dxrl_pg_log_row_world``), over the global sample count; env_steps advances by the
    global sample count.  Tables, headers, keep-best decisions and best parameters are therefore
    bit-identical on all ranks, so the polls of stop_on_converge / stop_on_patience decide the same
    on every rank and need no further collective: all ranks must call fit with the same arguments.
    Every rank runs the whole validation plan against its own (identical) weights.
    ``log.ranks`` keeps the ranks' records of every row.  On a trainer without a process group it
    takes the same path at world 1 with no collective and writes dxrl_pg_log_row's bytes.  A run
    is merged or not from its first row on."""
    if tr.collective and not merge_ranks:
        raise ValueError("fit() runs on one rank: on a collective trainer (world > 1 or a process group) pass "
                         "merge_ranks=True, which merges the ranks' log sums on the device between the reduce and "
                         "the finish stage")
    iterations = int(iterations)
    if iterations < 0 or int(poll_every) < 0:
        raise ValueError("iterations and poll_every must be >= 0")
    score_col = column_index(keep_best, "keep_best")
    conv_col, window, threshold = -1, 1, 0.0
    if converge is not None:
        name, window, threshold = converge
        conv_col, window, threshold = column_index(name, "converge column"), int(window), float(threshold)
        if name is None or window < 1:
            raise ValueError("converge must be (column, window >= 1, threshold)")
    if stop_on_converge and converge is None:
        raise ValueError("stop_on_converge needs converge=(column, window, threshold)")
    every, patience = int(validate_every), int(patience)
    if validation is not None and not isinstance(validation, ValidationPlan):
        raise ValueError("validation must be a ValidationPlan (tr.validation_plan(heldout_set, ...))")
    val_table, val_col = val_score(val_keep_best, validation is not None and validation.L > 0)
    if every < 1 or patience < 0:
        raise ValueError("validate_every must be >= 1 and patience >= 0")
    if stop_on_patience and (validation is None or patience < 1):
        raise ValueError("stop_on_patience needs validation=plan and patience >= 1")
    st = run_state(tr)
    merge_ranks = bool(merge_ranks)
    if st.rows and st.merged != merge_ranks:
        raise ValueError(f"this run's {st.rows} rows were logged with merge_ranks={st.merged}: a run keeps the "
                         "setting of its first row")
    if merge_ranks:
        st.merge_ranks(tr)
    val = val_state(tr, st, validation) if validation is not None else None
    st.reserve(tr, st.rows + iterations)
    if converge is not None:
        st.window = window
    st.settings = {"keep_best": keep_best, "min_episodes": int(min_episodes),
                   "converge": None if converge is None else [converge[0], window, threshold]}
    if val is not None:
        val.reserve(val.rows + iterations // every + 1)
        val.settings = {"validate_every": every, "val_keep_best": val_keep_best, "min_delta": float(min_delta),
                        "patience": patience}

    def validate():
        validation.run(tr, val, tr.iteration_index - 1, st.env_steps, st.rows - 1, val_col, min_delta, patience,
                       score_table=val_table)

    for k in range(iterations):
        if st.controlled:  # the iteration's last optimiser launch writes its row into the table
            tr._opt_row_target = st.opt_table[st.rows]
        if st.popart:  # likewise the iteration's rescale launch
            tr._vnorm_row_target = st.vnorm_table[st.rows]
        try:
            tr.iteration()
        finally:
            tr._opt_row_target = None
            if st.popart:
                tr._vnorm_row_target = None
        log_iteration(tr, st, score_col, min_episodes, conv_col, window, threshold, merge_ranks)
        validated = val is not None and (st.rows % every == 0 or k == iterations - 1)
        if validated:
            validate()
        if poll_every and (stop_on_converge or stop_on_patience) and (k + 1) % int(poll_every) == 0:
            st.host_reads += 1
            stop = stop_on_converge and header_dict(st.header.cpu().numpy())["converged_row"] >= 0
            if stop_on_patience and val_header_dict(val.header.cpu().numpy())["stopped_row"] >= 0:
                stop = True
            if stop:
                if val is not None and not validated:
                    validate()  # the last iteration of the run is always validated
                break
    return training_log(tr)


def training_log(tr) -> TrainingLog:
    """The run's log so far: one asynchronous copy into pinned memory, waited for on first use."""
    st = run_state(tr)
    last = st.last_log() if st.last_log is not None else None
    if last is not None:
        last._resolve()  # an earlier log still waiting for its copy takes it before the staging is reused
    if st.rows:
        st.host_table[:st.rows].copy_(st.table[:st.rows], non_blocking=True)
    if st.merged and st.rows:
        st.host_rank_log[:st.rows].copy_(st.rank_log[:st.rows], non_blocking=True)
    if st.controlled and st.rows:
        st.host_opt_table[:st.rows].copy_(st.opt_table[:st.rows], non_blocking=True)
    if st.popart and st.rows:
        st.host_vnorm_table[:st.rows].copy_(st.vnorm_table[:st.rows], non_blocking=True)
    st.host_header.copy_(st.header, non_blocking=True)
    st.event.record(torch.cuda.current_stream(tr.dev))
    log = TrainingLog(window=st.window, settings=st.settings,
                      _pending=(st.event, st.host_table, st.host_header, st.rows,
                                st.host_rank_log if st.merged else None,
                                st.host_opt_table if st.controlled else None,
                                st.host_vnorm_table if st.popart else None), validation=validation_log(tr))
    st.last_log = weakref.ref(log)
    return log


def best_policy(tr, deterministic: bool = True, seed: Optional[int] = None, which: str = "training"):
    """The actor of the best logged iteration (which="training") or of the best validation
    (which="validation") as a frozen ``MLPActorPolicy``."""
    from .policies import MLPActorPolicy
    if which not in ("training", "validation"):
        raise ValueError(f'which must be "training" or "validation", got {which!r}')
    st = getattr(tr, "_run", None)
    if which == "validation":
        if st is None or st.val is None or val_header_dict(st.val.header.cpu().numpy())["best_row"] < 0:
            raise ValueError("no validation-best parameters yet: run fit(validation=plan) with val_keep_best")
        return MLPActorPolicy.from_params(st.val.best_params, deterministic=deterministic, seed=seed)
    if st is None or header_dict(st.header.cpu().numpy())["best_row"] < 0:
        raise ValueError("no best parameters yet: run fit() with keep_best, and min_episodes that some iteration "
                         "reaches")
    return MLPActorPolicy.from_params(st.best_params, deterministic=deterministic, seed=seed)


# ====================================================================== checkpoints
def env_fingerprint(env) -> Dict[str, Any]:
    """The EnvConfig fields a slab depends on (max_episode_steps travels in the checkpoint)."""
    c = env._cfg
    out = {k: int(getattr(c, k)) for k in ("num_envs", "num_fingers", "joints_per_finger", "reward_type",
                                           "has_object_position", "seed", "global_env_offset")}
    out["object_position"] = [float(x) for x in c.object_position]
    out.update({k: float(getattr(c, k)) for k in ("distance_weight", "contact_weight", "closure_weight",
                                                  "stability_weight")})
    out["slab_bytes"] = int(env.layout.total_bytes)
    return out


def _config_state(c) -> Dict[str, Any]:
    from .experiments import CurriculumConfig
    return c.to_state() if hasattr(c, "to_state") else CurriculumConfig(**c.to_dict()).to_state()


def write_checkpoint(path, arrays: Dict[str, np.ndarray], meta: Dict[str, Any]):
    """One .npz: the arrays and `meta` as one JSON string (no pickle)."""
    meta = dict(meta, format=CHECKPOINT_FORMAT)
    with open(path, "wb") as f:
        np.savez(f, meta=np.array(json.dumps(meta)), **arrays)


def read_checkpoint(path):
    with np.load(path, allow_pickle=False) as z:
        if "meta" not in z.files:
            raise ValueError(f"{path}: not a {CHECKPOINT_FORMAT} file")
        meta = json.loads(str(z["meta"]))
        if meta.get("format") != CHECKPOINT_FORMAT:
            raise ValueError(f"{path}: not a {CHECKPOINT_FORMAT} file")
        return {k: z[k] for k in z.files if k != "meta"}, meta


def _rank_of(tr) -> int:
    if not tr.collective:
        return 0
    import torch.distributed as dist
    return dist.get_rank(tr.pg) if tr.pg is not None else dist.get_rank()


def save_checkpoint(tr, path):
    """This trainer's checkpoint; on a collective trainer this rank's file (ranks differ in env slab,
    running returns and global_env_offset), with the world size and the rank in its JSON part."""
    env = tr.env
    st = getattr(tr, "_run", None)
    torch.cuda.synchronize(tr.dev)
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    arrays = {"params": host(tr.params), "m1": host(tr.m1), "m2": host(tr.m2),
              "packed": host(tr.packed.view(torch.int16)), "ep_ret": host(tr.ep_ret),
              "env_state": host(env.state)}
    meta: Dict[str, Any] = {
        "step_count": int(tr.step_count), "iteration_index": int(tr.iteration_index),
        "trainer_config": _trainer_config_state(tr.cfg),
        "env": env_fingerprint(env), "max_episode_steps": int(env.max_episode_steps),
        "curriculum_configs": [_config_state(c) for c in env.curriculum_configs],
        "scheduler": tr.scheduler.get_state() if tr.scheduler is not None else None,
        "log": None,
    }
    if tr.lr_control:  # optional entry: a trainer without step-size control writes the file it always did
        arrays["opt_state"] = host(tr.opt_state)
    if tr.cfg.value_norm:  # likewise: the running return moments and the next iteration's (mu, sigma)
        arrays["value_norm_state"] = host(tr.vnorm)
    if tr.cfg.popart:  # likewise: the units the critic's head puts out
        arrays["popart_state"] = host(tr.popart)
    if st is not None:
        arrays.update(log_table=host(st.table[:st.rows]), log_header=host(st.header),
                      best_params=host(st.best_params))
        if st.controlled:
            arrays["log_optimizer"] = host(st.opt_table[:st.rows])
        if st.popart:
            arrays["log_value_norm"] = host(st.vnorm_table[:st.rows])
        meta["log"] = {"rows": st.rows, "env_steps": st.env_steps, "window": st.window, "settings": st.settings}
        if st.merged:  # optional entries: a run without merge_ranks writes the file it always did
            arrays["log_ranks"] = host(st.rank_log[:st.rows])
            meta["log"]["merge_ranks"] = True
        if st.val is not None:  # optional entries: a run never validated writes the file it always did
            v = st.val
            arrays.update(validation_arrays(host(v.table[:v.rows]), host(v.header), host(v.best_params),
                                            host(v.objects[:v.rows]),
                                            host(v.levels[:v.rows]) if v.L else None,
                                            host(v.robust[:v.rows]) if v.L else None,
                                            host(v.paired[:v.rows]) if v.crn else None,
                                            host(v.object_lost[:v.rows]) if v.crn else None,
                                            failure={name: host(getattr(v, name)[:v.rows]) for name in
                                                     v.optional_tables() if name.startswith("failure_")}))
            meta["validation"] = validation_meta(st.val.rows, st.val.fingerprint, st.val.object_names, st.val.settings)
    if tr.collective:  # likewise optional: a one-rank trainer writes the file it always did
        meta["world"], meta["rank"] = int(tr.world), _rank_of(tr)
    write_checkpoint(path, arrays, meta)


def _trainer_config_state(cfg) -> Dict[str, Any]:
    """The checkpoint's trainer_config: the dataclass's fields, without the step-size fields,
    timeout_bootstrap and the value-normalisation fields where they sit at their defaults (a trainer
    without them writes the entry it always did; a missing field loads as its default)."""
    from .lr_control import CONFIG_DEFAULTS
    from .value_norm import CONFIG_DEFAULTS as VALUE_NORM_DEFAULTS
    later = dict(CONFIG_DEFAULTS, timeout_bootstrap=False, **VALUE_NORM_DEFAULTS)
    d = dataclasses.asdict(cfg)
    return {k: v for k, v in d.items() if k not in later or v != later[k]}


def validation_arrays(table, header, best_params, objects, levels=None, robust=None, paired=None,
                      object_lost=None, failure=None) -> Dict[str, np.ndarray]:
    """The checkpoint's optional validation arrays (levels / robust: a plan with noise levels;
    paired / object_lost: one with common random numbers; failure: name -> array of the failure
    tables of a plan with failure modes)."""
    out = {"val_table": table, "val_header": header, "val_best_params": best_params, "val_objects": objects}
    if levels is not None:
        out.update(val_levels=levels, val_robust=robust)
    if paired is not None:
        out.update(val_paired=paired, val_object_lost=object_lost)
    for name, array in (failure or {}).items():
        out["val_" + name] = array
    return out


def validation_meta(rows: int, fingerprint, object_names, settings) -> Dict[str, Any]:
    """The checkpoint's optional `validation` entry of the JSON part."""
    return {"rows": int(rows), "fingerprint": fingerprint, "object_names": list(object_names),
            "settings": dict(settings or {})}


def validation_log_of_checkpoint(arrays: Dict[str, np.ndarray], meta: Dict[str, Any]) -> Optional[ValidationLog]:
    """The validation curve a checkpoint carries (None: the run was never validated, or the file
    predates validation)."""
    v = meta.get("validation")
    if v is None:
        return None
    noise = v["fingerprint"].get("noise_levels")  # absent: a plan without levels, or an older file
    crn = noise is not None and bool(v["fingerprint"].get("common_random_numbers"))  # absent likewise
    failures = v["fingerprint"].get("failure_modes") is not None  # absent likewise
    return ValidationLog(arrays["val_table"], val_header_dict(arrays["val_header"]), arrays["val_objects"],
                         v["object_names"], v.get("settings"), noise_levels=noise,
                         levels=arrays["val_levels"] if noise is not None else None,
                         robust=arrays["val_robust"] if noise is not None else None,
                         paired=arrays["val_paired"] if crn else None,
                         object_lost=arrays["val_object_lost"] if crn else None,
                         failure_modes=arrays["val_failure_modes"] if failures else None,
                         failure_levels=arrays["val_failure_levels"] if failures else None,
                         failure_transitions=arrays["val_failure_transitions"] if failures and crn else None)


def load_checkpoint(cls, path, env, process_group=None, world_size: int = 1):
    """A trainer on `env` continuing the checkpointed run.  `env` must have been built with the
    checkpoint's EnvConfig (ValueError otherwise); its state, curriculum table and episode
    limit are overwritten with the checkpoint's.  process_group / world_size: the collective
    trainer of a sharded run, each rank from its own file (the env's global_env_offset is part of
    the fingerprint); ValueError when the checkpoint was written at another world size."""
    from .experiments import CurriculumConfig, scheduler_from_state
    from .trainer import TrainerConfig
    arrays, meta = read_checkpoint(path)
    if int(meta.get("world", 1)) != int(world_size):  # absent: a one-rank trainer, or an older file
        raise ValueError(f"{path}: the checkpoint was written by rank {meta.get('rank', 0)} of a run over "
                         f"{meta.get('world', 1)} ranks, and world_size is {world_size}: a sharded run resumes at "
                         "the world size it was saved at")
    want, have = meta["env"], env_fingerprint(env)
    if want != have:
        diff = sorted(k for k in set(want) | set(have) if want.get(k) != have.get(k))
        raise ValueError(f"{path}: the checkpoint was written for another env configuration (differs in "
                         f"{', '.join(diff)})")
    cfg = dict(meta["trainer_config"])
    cfg["betas"] = tuple(cfg["betas"])
    from .value_norm import check_checkpoint, check_forget, check_popart_checkpoint
    check_checkpoint(bool(cfg.get("value_norm", False)), "value_norm_state" in arrays, path)
    check_popart_checkpoint(bool(cfg.get("popart", False)), "popart_state" in arrays, path)
    if "value_norm_state" in arrays:
        check_forget(cfg.get("value_norm_forget", 0.0), arrays["value_norm_state"], path)
    tr = cls(env, TrainerConfig(**cfg), process_group=process_group, world_size=world_size)
    if tr.collective and int(meta.get("rank", 0)) != _rank_of(tr):
        raise ValueError(f"{path}: the checkpoint of rank {meta.get('rank', 0)}, loaded on rank {_rank_of(tr)}")
    env.max_episode_steps = int(meta["max_episode_steps"])
    tr.max_steps = tr.cfg.max_steps or env.max_episode_steps
    if meta["scheduler"] is not None:
        tr.attach_curriculum(scheduler_from_state(meta["scheduler"]))
    configs = [CurriculumConfig.from_state(c) for c in meta["curriculum_configs"]]
    if meta["scheduler"] is None or len(configs) != 1:
        env.set_curricula(configs)  # the rows' count lives in the handle; the slab below carries the rest
    dev = tr.dev
    put = lambda dst, name: dst.copy_(torch.from_numpy(arrays[name]).to(dev).view(dst.dtype).view_as(dst))  # noqa: E731
    put(env.state, "env_state")
    for name in ("params", "m1", "m2", "ep_ret"):
        put(getattr(tr, name), name)
    put(tr.packed, "packed")
    tr._h2a_fresh = tr._h2c_fresh = False
    tr.step_count, tr.iteration_index = int(meta["step_count"]), int(meta["iteration_index"])
    if tr.lr_control:
        put(tr.opt_state, "opt_state")
    if tr.cfg.value_norm:
        put(tr.vnorm, "value_norm_state")
    if tr.cfg.popart:
        put(tr.popart, "popart_state")
    if meta["log"] is not None:
        lg = meta["log"]
        st = run_state(tr, int(lg["rows"]))
        st.rows, st.env_steps, st.window = int(lg["rows"]), int(lg["env_steps"]), lg["window"]
        st.settings = dict(lg["settings"] or {})
        if st.rows:
            put(st.table[:st.rows], "log_table")
        put(st.header, "log_header")
        put(st.best_params, "best_params")
        if st.controlled and st.rows:
            put(st.opt_table[:st.rows], "log_optimizer")
        if st.popart and st.rows:
            put(st.vnorm_table[:st.rows], "log_value_norm")
        if lg.get("merge_ranks"):  # absent in runs without merge_ranks and in older files
            st.merge_ranks(tr)
            if st.rows:
                put(st.rank_log[:st.rows], "log_ranks")
        v = meta.get("validation")  # absent in checkpoints written before validation existed
        if v is not None:
            val = st.val = _ValState(tr, v["fingerprint"], v["object_names"], int(v["rows"]))
            val.rows, val.settings = int(v["rows"]), dict(v["settings"] or {})
            if val.rows:
                put(val.table[:val.rows], "val_table")
                put(val.objects[:val.rows], "val_objects")
                if val.L:
                    put(val.levels[:val.rows], "val_levels")
                    put(val.robust[:val.rows], "val_robust")
                if val.crn:
                    put(val.paired[:val.rows], "val_paired")
                    put(val.object_lost[:val.rows], "val_object_lost")
                for name in val.optional_tables():
                    if name.startswith("failure_"):
                        put(getattr(val, name)[:val.rows], "val_" + name)
            put(val.header, "val_header")
            put(val.best_params, "val_best_params")
    torch.cuda.synchronize(dev)
    return tr
