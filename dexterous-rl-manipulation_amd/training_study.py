"""Studies of the policy-gradient trainer: a set of ``PGTrainer.fit`` runs (arms x seeds) and the
reduction of their device tables to per-run rows, per-arm tables and effects paired by seed.

``run_training_study`` is the layer above one run.  Every (arm, seed) job is a fresh ``VecEnv`` and
``PGTrainer`` (``make_job``: env and trainer seeded as ``reward_comparison.run_training_comparison``
seeds them, a curriculum arm with ``ablation.study_scheduler`` attached, every job with the same
held-out validation plan) that runs as one ``fit``.  Jobs run one after another -- the learner
kernels fill the GPU.  After a job its training log and its validation table are copied device to
device into the study's two slabs (``f64 [runs][cap][cols]``) on the trainer's stream; the trainer is
then released (releasing an env waits for the stream; nothing is read back).  At the end one
``dxrl_pg_runs_summarize`` call per slab (csrc/dxrl_pg_runs.hip) writes

* ``run_table  [R][S][8]``: per run and spec -- rows, final_window_mean, best, best_row,
  convergence_row (``dxrl_pg_log_row``'s rule), x_at_convergence, curve_mean, nan_rows;
* ``group_table [G][S][5][6]``: per arm, spec and metric over the arm's seeds -- count, mean,
  population std (``compute_ablation_statistics``' ``np.std``), min, max, converged runs;
* ``contrast_table [Q][S][5][5]``: per contrast (a weight per arm; runs paired by seed) -- pairs,
  mean, sample std, standard error, mean / standard error.

A spec is a column of the slab with the convergence rule applied to it (``Spec``).  The validation
slab is the yardstick across arms: its success rate is measured on the same held-out episodes
under both rewards and under any training curriculum.  ``device_summary=False`` copies the slabs
to the host and computes the same three tables with NumPy (``summarize_host``) -- the path the
device one is tested and timed against.

One rank only: a collective trainer raises (sharded runs are open; so are arms side by side on one
GPU, plots and medians).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N

STUDY_FORMAT = "dxrl-training-study-v1"
RUN_COLUMNS = N.PG_RUNS_RUN_COLUMNS
METRICS = N.PG_RUNS_METRICS
GROUP_COLUMNS = N.PG_RUNS_GROUP_COLUMNS
CONTRAST_COLUMNS = N.PG_RUNS_CONTRAST_COLUMNS
SLABS = ("training", "validation")
_SLAB_COLUMNS = {"training": N.PG_LOG_COLUMNS, "validation": N.PG_VAL_COLUMNS}
_SLAB_COLS = {"training": N.PG_LOG_COLS, "validation": N.PG_VAL_COLS}
_WAVE = 64
# run-table column of every metric (enum dxrl_pg_runs_metric -> enum dxrl_pg_runs_run_col)
_METRIC_RUN_COL = tuple(RUN_COLUMNS.index(m) for m in METRICS)
_CONV = RUN_COLUMNS.index("convergence_row")


@dataclass
class Arm:
    """One arm of a study: with ``use_curriculum`` the trainer gets
    ``ablation.study_scheduler(scheduler_config)`` attached (and starts on its initial config),
    otherwise it trains on the fixed ``curriculum`` preset.  ``trainer_kw`` goes to
    ``TrainerConfig`` on top of the study's own."""
    name: str
    use_curriculum: bool
    reward_type: str
    curriculum: str = "hard"
    scheduler_config: Any = None
    trainer_kw: Dict[str, Any] = field(default_factory=dict)


@dataclass(frozen=True)
class Spec:
    """A column of a slab and the convergence rule on it: converged at the first row whose mean
    over the last ``window`` rows is strictly above ``threshold`` (``x_column`` is reported at that
    row); ``final_window`` rows make the final mean."""
    column: str
    x_column: str = "env_steps"
    window: int = 10
    threshold: float = 0.5
    final_window: int = 10


DEFAULT_TRAIN_SPECS = (Spec("success_rate"), Spec("mean_length"), Spec("mean_return"))
DEFAULT_VAL_SPECS = (Spec("success_rate"), Spec("mean_length"), Spec("mean_return"))


def _check_specs(specs: Sequence[Spec], slab: str) -> Tuple[Spec, ...]:
    specs = tuple(specs)
    names = _SLAB_COLUMNS[slab]
    if not 1 <= len(specs) <= N.PG_RUNS_MAX_SPECS:
        raise ValueError(f"a {slab} summary takes 1 .. {N.PG_RUNS_MAX_SPECS} specs, got {len(specs)}")
    for s in specs:
        if s.column not in names or s.x_column not in names:
            raise ValueError(f"{slab} spec {s}: column and x_column must be among {list(names)}")
        if int(s.window) < 1 or int(s.final_window) < 1:
            raise ValueError(f"{slab} spec {s}: window and final_window must be >= 1")
    return specs


def native_specs(specs: Sequence[Spec], slab: str):
    """The ``dxrl_pg_runs_spec`` array of a slab's specs."""
    names = _SLAB_COLUMNS[slab]
    arr = (N.PgRunsSpec * len(specs))()
    for k, s in enumerate(specs):
        arr[k].col, arr[k].x_col = names.index(s.column), names.index(s.x_column)
        arr[k].window, arr[k].final_window, arr[k].threshold = int(s.window), int(s.final_window), float(s.threshold)
    return arr


# ====================================================================== the NumPy path
def _push(m, x):
    n1 = m[0] + 1.0
    d = x - m[1]
    mean = m[1] + d / n1
    return (n1, mean, m[2] + d * (x - mean))


def _merge(a, b):
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n = a[0] + b[0]
    d = b[1] - a[1]
    return (n, a[1] + d * (b[0] / n), a[2] + b[2] + d * d * (a[0] * b[0] / n))


def _wave_moments(values):
    """The (count, mean, M2) of `values` in the device's order: lane t takes positions t, t + 64,
    .. as Welford steps (a None or a non-finite value at a position is a step not taken), the 64
    triples merge in the tree offsets 32, .., 1."""
    lanes = [(0.0, 0.0, 0.0)] * _WAVE
    for j, x in enumerate(values):
        if x is not None and math.isfinite(x):
            lanes[j % _WAVE] = _push(lanes[j % _WAVE], float(x))
    o = _WAVE // 2
    while o:
        for t in range(o):
            lanes[t] = _merge(lanes[t], lanes[t + o])
        o //= 2
    return lanes[0]


def _run_row(v: np.ndarray, x: np.ndarray, spec) -> np.ndarray:
    """One run-table row from the run's column `v` and x column `x` (n rows each)."""
    n, W, FW, thr = len(v), int(spec.window), int(spec.final_window), float(spec.threshold)
    out = np.full(len(RUN_COLUMNS), np.nan)
    out[0] = n
    k = min(FW, n)
    if k:
        s = 0.0
        for y in v[n - k:]:
            s = s + float(y)
        out[1] = s / k
    ok = ~np.isnan(v)
    out[3] = -1.0
    if ok.any():
        best = v[ok].max()
        out[2], out[3] = best, int(np.flatnonzero(ok & (v == best))[0])
    out[4] = -1.0
    for i in range(W - 1, n):
        s = 0.0
        for y in v[i - W + 1:i + 1]:
            s = s + float(y)
        if s / W > thr:
            out[4], out[5] = i, x[i]
            break
    if ok.any():
        part = np.zeros(_WAVE)
        for i in np.flatnonzero(ok):
            part[i % _WAVE] += v[i]
        o = _WAVE // 2
        while o:
            part[:o] += part[o:2 * o]
            o //= 2
        out[6] = part[0] / int(ok.sum())
    out[7] = int((~ok).sum())
    return out


def _metrics_of(run_row: np.ndarray) -> np.ndarray:
    x = run_row[list(_METRIC_RUN_COL)].copy()
    if run_row[_CONV] < 0:
        x[METRICS.index("convergence_row")] = np.nan
    return x


def summarize_host(tables: np.ndarray, run_rows: Sequence[int], specs, group_offsets: Sequence[int] = (0,),
                   group_runs: Sequence[int] = (), contrast_weights=None):
    """``dxrl_pg_runs_summarize`` in NumPy, in the orders include/dxrl.h states: returns
    ``(run_table, group_table, contrast_table, status)``.  `specs`: objects with col, x_col, window,
    final_window and threshold (``native_specs``)."""
    tables = np.asarray(tables, dtype=np.float64)
    R, cap, _ = tables.shape
    S, G = len(specs), len(group_offsets) - 1
    W = np.zeros((0, G)) if contrast_weights is None else np.asarray(contrast_weights, dtype=np.float64).reshape(-1, G)
    Q, M = len(W), len(group_runs)
    status = 0
    run_table = np.zeros((R, S, len(RUN_COLUMNS)))
    for r in range(R):
        n = int(run_rows[r])
        if n < 0 or n > cap:
            status |= N.PG_RUNS_ST_ROWS
            n = 0
        for s, sp in enumerate(specs):
            run_table[r, s] = _run_row(tables[r, :n, sp.col], tables[r, :n, sp.x_col], sp)

    def members(g):
        lo, hi = int(group_offsets[g]), int(group_offsets[g + 1])
        return None if lo < 0 or hi < lo or hi > M else [int(x) for x in group_runs[lo:hi]]

    group_table = np.full((G, S, len(METRICS), len(GROUP_COLUMNS)), np.nan)
    for g in range(G):
        mem = members(g)
        if mem is None:
            status |= N.PG_RUNS_ST_RANGE
            mem = []
        if any(r < 0 or r >= R for r in mem):
            status |= N.PG_RUNS_ST_RANGE
        for s in range(S):
            # position j of the group is a step of lane j % 64; an out-of-range member takes none
            x = [_metrics_of(run_table[r, s]) if 0 <= r < R else None for r in mem]
            conv = sum(1 for r in mem if 0 <= r < R and run_table[r, s, _CONV] >= 0)
            for k in range(len(METRICS)):
                vals = [None if xr is None else float(xr[k]) for xr in x]
                n, mean, m2 = _wave_moments(vals)
                fin = [v for v in vals if v is not None and math.isfinite(v)]
                group_table[g, s, k, 0], group_table[g, s, k, 5] = n, conv
                if n:
                    group_table[g, s, k, 1:5] = mean, math.sqrt(m2 / n), min(fin), max(fin)
    contrast_table = np.full((Q, S, len(METRICS), len(CONTRAST_COLUMNS)), np.nan)
    for q in range(Q):
        used = [g for g in range(G) if W[q, g] != 0.0]
        mems = [members(g) for g in used]
        sizes = {len(m) for m in mems if m is not None}
        if any(m is None for m in mems) or len(sizes) > 1:
            status |= N.PG_RUNS_ST_CONTRAST
            continue
        m = sizes.pop() if sizes else 0
        for s in range(S):
            for k in range(len(METRICS)):
                vals = []
                for j in range(m):
                    d, ok = 0.0, True
                    for g, mem in zip(used, mems):
                        r = mem[j]
                        if r < 0 or r >= R:
                            ok = False
                            continue
                        with np.errstate(invalid="ignore", over="ignore"):
                            term = W[q, g] * _metrics_of(run_table[r, s])[k]
                        ok = ok and bool(np.isfinite(term))
                        d = d + term
                    vals.append(d if ok else None)
                n, mean, m2 = _wave_moments(vals)
                row = contrast_table[q, s, k]
                row[0] = n
                if n:
                    sd = math.sqrt(m2 / (n - 1.0)) if n >= 2 else float("nan")
                    se = sd / math.sqrt(n)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        row[1:] = mean, sd, se, np.float64(mean) / np.float64(se)
    return run_table, group_table, contrast_table, status


# ====================================================================== the summary of one slab
class SlabSummary:
    """The three tables of one slab with named accessors; after a device summary they are copied
    once, when first read (as ``TrainingLog``)."""

    def __init__(self, slab: str, specs: Sequence[Spec], run_names, group_names, contrast_names, run_table=None,
                 group_table=None, contrast_table=None, status: int = 0, _pending=None):
        self.slab, self.specs = slab, tuple(specs)
        self.run_names, self.group_names = list(run_names), list(group_names)
        self.contrast_names = list(contrast_names)
        R, S, G, Q = len(self.run_names), len(self.specs), len(self.group_names), len(self.contrast_names)
        self._shapes = ((R, S, len(RUN_COLUMNS)), (G, S, len(METRICS), len(GROUP_COLUMNS)),
                        (Q, S, len(METRICS), len(CONTRAST_COLUMNS)))
        self._pending = _pending
        self._tables = None
        if _pending is None:
            self._tables = tuple(np.array(t, dtype=np.float64).reshape(shape) for t, shape in
                                 zip((run_table, group_table, contrast_table), self._shapes))
            self._status = int(status)

    def _resolve(self):
        if self._pending is not None:
            event, host, status = self._pending
            event.synchronize()
            flat, at, tables = host.numpy(), 0, []
            for shape in self._shapes:
                size = int(np.prod(shape))
                tables.append(flat[at:at + size].reshape(shape).copy())
                at += size
            self._tables, self._status = tuple(tables), int(status.numpy()[0])
            self._pending = None

    @property
    def run_table(self) -> np.ndarray:
        self._resolve()
        return self._tables[0]

    @property
    def group_table(self) -> np.ndarray:
        self._resolve()
        return self._tables[1]

    @property
    def contrast_table(self) -> np.ndarray:
        self._resolve()
        return self._tables[2]

    @property
    def status(self) -> int:
        self._resolve()
        return self._status

    def spec_index(self, column: str) -> int:
        for k, s in enumerate(self.specs):
            if s.column == column:
                return k
        raise KeyError(f"the {self.slab} summary has no spec on {column!r} (it has "
                       f"{[s.column for s in self.specs]})")

    def run(self, column: str, name: str) -> np.ndarray:
        """[R]: one run-table column (RUN_COLUMNS) of the spec on `column`, in run order."""
        return self.run_table[:, self.spec_index(column), RUN_COLUMNS.index(name)]

    def group(self, group: str, column: str, metric: str) -> Dict[str, float]:
        """{count, mean, std, min, max, num_converged} of `metric` (METRICS) over a group's runs."""
        row = self.group_table[self.group_names.index(group), self.spec_index(column), METRICS.index(metric)]
        return {k: float(row[j]) for j, k in enumerate(GROUP_COLUMNS)}

    def contrast(self, contrast: str, column: str, metric: str) -> Dict[str, float]:
        """{pairs, mean, std, stderr, t} of `metric` for one contrast."""
        row = self.contrast_table[self.contrast_names.index(contrast), self.spec_index(column),
                                  METRICS.index(metric)]
        return {k: float(row[j]) for j, k in enumerate(CONTRAST_COLUMNS)}

    def to_dict(self) -> Dict[str, Any]:
        enc = lambda t: _encode(t.tolist())  # noqa: E731
        return {"specs": [dataclasses.asdict(s) for s in self.specs], "status": self.status,
                "run_columns": list(RUN_COLUMNS), "metrics": list(METRICS), "group_columns": list(GROUP_COLUMNS),
                "contrast_columns": list(CONTRAST_COLUMNS), "run_table": enc(self.run_table),
                "group_table": enc(self.group_table), "contrast_table": enc(self.contrast_table)}


def _encode(x):
    """NaN and the infinities as strings (``TrainingLog.to_dict``'s convention): standard JSON."""
    if isinstance(x, list):
        return [_encode(y) for y in x]
    if isinstance(x, float) and not math.isfinite(x):
        return "nan" if math.isnan(x) else ("inf" if x > 0 else "-inf")
    return x


class StudyResult:
    """What ``run_training_study`` returns: the arms, seeds and run order (run ``a * len(seeds) +
    k`` is arm a, seed k), ``training`` and ``validation`` (``SlabSummary``; validation None when
    no validation ran), per run the scheduler's final progression step (None for a fixed arm) and
    the host reads made inside ``fit``, the bytes the summaries copied to the host, and ``logs``
    (the runs' ``TrainingLog``s) when asked for."""

    def __init__(self, arms: Sequence[str], seeds: Sequence[int], iterations: int, training: SlabSummary,
                 validation: Optional[SlabSummary], contrasts: Dict[str, Dict[str, float]],
                 progression_steps: Sequence[Optional[int]] = (), host_reads: Sequence[int] = (),
                 bytes_copied: int = 0, device_summary: bool = True, logs=None, settings=None, slabs=None,
                 run_rows=None):
        self.slabs = dict(slabs or {})        # name -> the device slab f64 [R][cap][cols] (a study that ran)
        self.run_rows = {k: list(v) for k, v in (run_rows or {}).items()}  # name -> rows written per run
        self.arms, self.seeds, self.iterations = list(arms), [int(s) for s in seeds], int(iterations)
        self.training, self.validation = training, validation
        self.contrasts = {k: dict(v) for k, v in contrasts.items()}
        self.progression_steps, self.host_reads = list(progression_steps), list(host_reads)
        self.bytes_copied, self.device_summary = int(bytes_copied), bool(device_summary)
        self.logs = logs
        self.settings = dict(settings or {})

    @property
    def run_names(self) -> List[Tuple[str, int]]:
        return [(a, s) for a in self.arms for s in self.seeds]

    def run_index(self, arm: str, seed: int) -> int:
        return self.arms.index(arm) * len(self.seeds) + self.seeds.index(int(seed))

    def slab(self, name: str) -> SlabSummary:
        if name not in SLABS:
            raise ValueError(f"a slab is one of {list(SLABS)}, got {name!r}")
        s = getattr(self, name)
        if s is None:
            raise ValueError("this study ran without validation")
        return s

    @property
    def yardstick(self) -> SlabSummary:
        """The validation summary when a validation ran, else the training one."""
        return self.validation if self.validation is not None else self.training

    def status(self) -> Dict[str, int]:
        return {name: self.slab(name).status for name in SLABS if getattr(self, name) is not None}

    def tables(self, name: str) -> np.ndarray:
        """A host copy of a slab, f64 [R][cap][cols] (a copy of its own, made when asked for): run
        r's rows are ``tables(name)[r, :run_rows[name][r]]``."""
        if name not in self.slabs:
            raise ValueError(f"this result holds no {name!r} slab")
        return self.slabs[name].cpu().numpy()

    def to_dict(self) -> Dict[str, Any]:
        out = {"format": STUDY_FORMAT, "arms": self.arms, "seeds": self.seeds, "iterations": self.iterations,
               "runs": [[a, s] for a, s in self.run_names], "contrasts": self.contrasts,
               "progression_steps": self.progression_steps, "host_reads": self.host_reads,
               "bytes_copied": self.bytes_copied, "device_summary": self.device_summary, "settings": self.settings,
               "training": self.training.to_dict(),
               "validation": None if self.validation is None else self.validation.to_dict()}
        if self.logs is not None:
            out["logs"] = [log.to_dict() for log in self.logs]
        return out

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2, allow_nan=False)


# ====================================================================== one job
def make_job(arm: Arm, seed: int, *, num_envs: int = 4096, horizon: int = 200, max_steps: int = 200,
             heldout_set=None, validate_every: int = 10, val_episodes: int = 5, val_seed: int = 0,
             val_max_steps: Optional[int] = None, train_spec: Spec = DEFAULT_TRAIN_SPECS[0], device=None,
             **trainer_kw):
    """The env, trainer and ``fit`` arguments of one (arm, seed) job: ``(env, tr, fit_kw)``, so
    that ``tr.fit(iterations, **fit_kw)`` is the job.  ``validate_every=0``: no validation;
    ``val_max_steps``: the step limit of a validation episode (default ``max_steps``)."""
    from .ablation import study_scheduler
    from .envs import VecEnv
    from .experiments import CurriculumConfig
    from .trainer import PGTrainer, TrainerConfig
    if arm.reward_type not in ("sparse", "dense"):
        raise ValueError(f"arm {arm.name!r}: reward_type must be 'sparse' or 'dense', got {arm.reward_type!r}")
    sched = study_scheduler(arm.scheduler_config) if arm.use_curriculum else None
    config = sched.get_current_config() if sched is not None else CurriculumConfig.named(arm.curriculum)
    env = VecEnv(num_envs, curriculum_config=config, reward_type=arm.reward_type, max_episode_steps=max_steps,
                 seed=seed, device=device)
    kw = dict(trainer_kw)
    kw.update(arm.trainer_kw)
    tr = PGTrainer(env, TrainerConfig(horizon=horizon, seed=seed, max_steps=max_steps, **kw))
    if tr.collective:
        raise ValueError("a training study runs on one rank")
    if sched is not None:
        tr.attach_curriculum(sched)
    env.reset(write_obs=False)
    fit_kw: Dict[str, Any] = dict(keep_best=train_spec.column,
                                  converge=(train_spec.column, int(train_spec.window), float(train_spec.threshold)))
    if validate_every:
        if heldout_set is None:
            from .evaluation import HeldOutObjectSet
            heldout_set = HeldOutObjectSet(CurriculumConfig.hard())
        plan = tr.validation_plan(heldout_set, episodes_per_object=val_episodes, seed=val_seed,
                                  max_steps=int(val_max_steps or max_steps))
        fit_kw.update(validation=plan, validate_every=int(validate_every))
    return env, tr, fit_kw


def release_job(env, tr, fit_kw):
    plan = fit_kw.get("validation")
    if plan is not None:
        plan.env.close()
    env.close()


# ====================================================================== the runner
def csr_groups(groups: Sequence[Sequence[int]]):
    off = np.zeros(len(groups) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(g) for g in groups])
    flat = np.concatenate([np.asarray(g, dtype=np.int32) for g in groups]) if off[-1] else np.zeros(0, np.int32)
    return off, flat


def contrast_matrix(arms: Sequence[str], contrasts: Optional[Dict[str, Dict[str, float]]]) -> np.ndarray:
    """f64 [Q][G]: a row of arm weights per contrast."""
    contrasts = contrasts or {}
    W = np.zeros((len(contrasts), len(arms)))
    for q, (name, weights) in enumerate(contrasts.items()):
        for arm, w in weights.items():
            if arm not in arms:
                raise ValueError(f"contrast {name!r} weighs {arm!r}, which is not an arm ({list(arms)})")
            W[q, list(arms).index(arm)] = float(w)
    return W


def summarize_device(slab, run_rows: Sequence[int], specs, group_offsets: np.ndarray, group_runs: np.ndarray,
                     weights: np.ndarray, stream: Optional[int] = None):
    """One ``dxrl_pg_runs_summarize`` call on a device slab f64 [R][cap][cols] (enqueued, no sync).
    Returns ``(pending, nbytes)``: the ``SlabSummary`` ``_pending`` tuple of the one asynchronous
    copy of the three tables and the status word, and its size."""
    import torch
    dev = slab.device
    R, cap, cols = slab.shape
    S, G, Q = len(specs), len(group_offsets) - 1, len(weights)
    sizes = (R * S * len(RUN_COLUMNS), G * S * len(METRICS) * len(GROUP_COLUMNS),
             Q * S * len(METRICS) * len(CONTRAST_COLUMNS))
    with torch.cuda.device(dev):
        out = torch.zeros(sum(sizes), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rows_d = torch.tensor(list(run_rows), dtype=torch.int32).to(dev)
        off_d = torch.from_numpy(np.ascontiguousarray(group_offsets, dtype=np.int32)).to(dev)
        mem_d = torch.from_numpy(np.ascontiguousarray(group_runs, dtype=np.int32)).to(dev)
        w_d = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).to(dev)
        a = N.PgRunsArgs()
        a.num_runs, a.cap, a.cols, a.num_specs = R, cap, cols, S
        a.num_groups, a.num_members, a.num_contrasts = G, len(group_runs), Q
        a.specs = specs
        a.tables, a.run_rows = N.ptr(slab), N.ptr(rows_d)
        a.group_offsets, a.group_runs = N.ptr(off_d), N.ptr(mem_d) if len(group_runs) else None
        a.contrast_weights = N.ptr(w_d) if Q else None
        a.run_table = out.data_ptr()
        a.group_table = out.data_ptr() + 8 * sizes[0] if G else None
        a.contrast_table = out.data_ptr() + 8 * (sizes[0] + sizes[1]) if Q else None
        a.status = N.ptr(status)
        s = torch.cuda.current_stream(dev)
        N.call("dxrl_pg_runs_summarize", dev.index, C.byref(a), s.cuda_stream if stream is None else stream)
        host = torch.zeros(sum(sizes), dtype=torch.float64).pin_memory()
        host_status = torch.zeros(1, dtype=torch.int32).pin_memory()
        host.copy_(out, non_blocking=True)
        host_status.copy_(status, non_blocking=True)
        event = torch.cuda.Event()
        event.record(s)
    return (event, host, host_status), 8 * sum(sizes) + 4


def run_training_study(arms: Sequence[Arm], seeds: Sequence[int], iterations: int, *, num_envs: int = 4096,
                       horizon: int = 200, max_steps: int = 200, heldout_set=None, validate_every: int = 10,
                       val_episodes: int = 5, val_seed: int = 0, val_max_steps: Optional[int] = None,
                       train_specs: Sequence[Spec] = DEFAULT_TRAIN_SPECS, val_specs: Sequence[Spec] = DEFAULT_VAL_SPECS,
                       contrasts: Optional[Dict[str, Dict[str, float]]] = None, device_summary: bool = True,
                       return_logs: bool = False, device=None, **trainer_kw) -> StudyResult:
    """Run every (arm, seed) job as one ``fit(iterations, keep_best=c, converge=(c, W, thr),
    validation=plan, validate_every=...)`` (c, W, thr: the first training spec's), keep the runs'
    tables in two device slabs and reduce each with one ``dxrl_pg_runs_summarize`` call.
    ``contrasts``: name -> {arm name: weight}; the weighted arms' runs are paired by seed.
    ``validate_every=0`` runs without validation (``StudyResult.validation`` is None);
    ``val_max_steps``: the step limit of a validation episode (default ``max_steps``).  The held-out
    set defaults to ``HeldOutObjectSet(CurriculumConfig.hard())``; ``trainer_kw`` goes to every
    job's ``TrainerConfig``."""
    import torch
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("a training study runs on one rank (sharded runs are not built): run it outside the "
                         "process group")
    arms, seeds, iterations = list(arms), [int(s) for s in seeds], int(iterations)
    if not arms or not seeds or iterations < 1:
        raise ValueError("a study needs at least one arm, one seed and one iteration")
    names = [a.name for a in arms]
    if len(set(names)) != len(names) or len(set(seeds)) != len(seeds):
        raise ValueError("arm names and seeds must be distinct")
    every = int(validate_every)
    if every < 0:
        raise ValueError("validate_every must be >= 0")
    train_specs = _check_specs(train_specs, "training")
    val_specs = _check_specs(val_specs, "validation") if every else ()
    weights = contrast_matrix(names, contrasts)
    dev = N.require_gpu(device)
    R = len(arms) * len(seeds)
    cap = {"training": iterations, "validation": iterations // every + 1 if every else 0}
    slabs = {k: torch.zeros(R, cap[k], _SLAB_COLS[k], dtype=torch.float64, device=dev) for k in SLABS if cap[k]}
    rows = {k: [0] * R for k in slabs}
    progression, host_reads, logs = [], [], []
    r = 0
    for arm in arms:
        for seed in seeds:
            env, tr, fit_kw = make_job(arm, seed, num_envs=num_envs, horizon=horizon, max_steps=max_steps,
                                       heldout_set=heldout_set, validate_every=every, val_episodes=val_episodes,
                                       val_seed=val_seed, val_max_steps=val_max_steps, train_spec=train_specs[0],
                                       device=dev, **trainer_kw)
            log = None
            try:
                log = tr.fit(iterations, **fit_kw)
                st = tr._run
                with torch.cuda.device(dev):  # device to device, behind the run on its stream
                    rows["training"][r] = st.rows
                    slabs["training"][r, :st.rows].copy_(st.table[:st.rows])
                    if every:
                        rows["validation"][r] = st.val.rows
                        slabs["validation"][r, :st.val.rows].copy_(st.val.table[:st.val.rows])
                progression.append(len(tr.scheduler.progression_history) if tr.scheduler is not None else None)
                host_reads.append(int(st.host_reads))
                if return_logs:
                    log.table  # the log's own copy, before its staging buffers go
                    if log.validation is not None:
                        log.validation.table
                    logs.append(log)
            finally:
                release_job(env, tr, fit_kw)
                del env, tr, fit_kw, log
            r += 1
    groups = [[a * len(seeds) + k for k in range(len(seeds))] for a in range(len(arms))]
    off, flat = csr_groups(groups)
    run_names = [(a, s) for a in names for s in seeds]
    summaries: Dict[str, Optional[SlabSummary]] = {"training": None, "validation": None}
    copied = 0
    for k, slab in slabs.items():
        specs = train_specs if k == "training" else val_specs
        nat = native_specs(specs, k)
        if device_summary:
            pending, nbytes = summarize_device(slab, rows[k], nat, off, flat, weights)
            summaries[k] = SlabSummary(k, specs, run_names, names, list(contrasts or {}), _pending=pending)
        else:
            host = slab.cpu().numpy()
            nbytes = host.nbytes
            rt, gt, ct, status = summarize_host(host, rows[k], nat, off, flat, weights)
            summaries[k] = SlabSummary(k, specs, run_names, names, list(contrasts or {}), rt, gt, ct, status)
        copied += nbytes
    settings = {"num_envs": int(num_envs), "horizon": int(horizon), "max_steps": int(max_steps),
                "validate_every": every, "val_episodes": int(val_episodes), "val_seed": int(val_seed),
                "val_max_steps": int(val_max_steps or max_steps),
                "arms": [{"name": a.name, "use_curriculum": bool(a.use_curriculum), "reward_type": a.reward_type,
                          "curriculum": a.curriculum} for a in arms]}
    return StudyResult(names, seeds, iterations, summaries["training"], summaries["validation"], contrasts or {},
                       progression, host_reads, copied, device_summary, logs if return_logs else None, settings,
                       slabs=slabs, run_rows=rows)


__all__ = ["Arm", "Spec", "StudyResult", "SlabSummary", "run_training_study", "make_job", "release_job", "csr_groups",
           "summarize_host",
           "summarize_device", "native_specs", "contrast_matrix", "DEFAULT_TRAIN_SPECS", "DEFAULT_VAL_SPECS"]
