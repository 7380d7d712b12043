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
_MIN_CAP = 256


def column_index(name: Optional[str], what: str) -> int:
    if name is None:
        return -1
    if name not in _SCORE_COLUMNS:
        raise ValueError(f"{what} must be one of {list(_SCORE_COLUMNS)} or None, got {name!r}")
    return COLUMNS.index(name)


# ====================================================================== TrainingLog
class TrainingLog:
    """The learning curve of a run: one row per iteration, named NumPy columns
    (``log["mean_return"]``, ``log.columns``), the best and the convergence iteration.

    ``best_iteration``: the ``iteration`` value of the row keep-best chose (None: no row
    qualified).  ``convergence_iteration``: the ``iteration`` value of row
    ``converged_row - W + 1``, the first row of the first window whose mean exceeded the
    threshold (reward_comparison.py:121-124), or None."""

    def __init__(self, table=None, header: Optional[Dict[str, Any]] = None, window: Optional[int] = None,
                 settings: Optional[Dict[str, Any]] = None, _pending=None):
        self._pending = _pending
        self._table = None if table is None else np.array(table, dtype=np.float64).reshape(-1, COLS)
        self._header = dict(header) if header is not None else None
        self.window = window
        self.settings = dict(settings or {})

    # -- lazy fill (fit enqueued the copy; the first read waits for it)
    def _resolve(self):
        if self._pending is not None:
            event, host_table, host_header, rows = self._pending
            event.synchronize()
            self._table = host_table[:rows].numpy().copy()
            self._header = header_dict(host_header.numpy())
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
        return {"format": LOG_FORMAT, "columns": list(COLUMNS), "window": self.window, "settings": self.settings,
                "header": {k: _enc(v) for k, v in self.header.items()},
                "rows": [[_enc(x) for x in row[:len(COLUMNS)]] for row in self.table.tolist()]}

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "TrainingLog":
        if d.get("format") != LOG_FORMAT or list(d.get("columns", [])) != list(COLUMNS):
            raise ValueError(f"not a {LOG_FORMAT} log with this build's columns")
        table = np.zeros((len(d["rows"]), COLS), dtype=np.float64)
        for r, row in enumerate(d["rows"]):
            table[r, :len(COLUMNS)] = [_dec(x) for x in row]
        return cls(table, {k: _dec(v) for k, v in d["header"].items()}, d.get("window"), d.get("settings"))

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
        self.reserve(tr, cap)

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


def run_state(tr, cap: int = 0) -> _RunState:
    st = getattr(tr, "_run", None)
    if st is None:
        st = tr._run = _RunState(tr, cap)
    else:
        st.reserve(tr, cap)
    return st


def log_iteration(tr, st: _RunState, score_col: int, min_episodes: int, conv_col: int, window: int,
                  threshold: float):
    """One dxrl_pg_log_row call for the iteration that just ran (enqueued, no sync)."""
    p = N.ptr
    a = N.PgLogArgs()
    a.num_envs, a.horizon, a.row, a.cap = tr.n, tr.T, st.rows, st.cap
    st.env_steps += tr.M
    a.iteration, a.env_steps = tr.iteration_index - 1, st.env_steps
    loss = tr.fused_loss if tr.cfg.fused else tr.loss_partial
    a.loss_blocks, a.loss_rows = loss.shape[0], (tr._loss_rows if tr.cfg.fused else tr.M)
    a.min_episodes, a.num_params, a.partial_doubles = int(min_episodes), tr.params.numel(), st.partial.numel()
    a.score_col, a.conv_col, a.conv_window, a.conv_threshold = score_col, conv_col, int(window), float(threshold)
    a.ep_count, a.ep_sum_return, a.ep_sum_length = p(tr.ep_count), p(tr.ep_sum_ret), p(tr.ep_sum_len)
    a.ep_successes, a.rew, a.ret, a.done, a.values = p(tr.ep_succ), p(tr.rew), p(tr.ret), p(tr.done), p(tr.V[0])
    a.stats, a.loss_partial, a.gnorm2 = p(tr.stats), p(loss), p(tr.gnorm2)
    a.params, a.best_params = p(tr.params), p(st.best_params)
    a.partial, a.log, a.header = p(st.partial), p(st.table), p(st.header)
    N.call("dxrl_pg_log_row", tr.dev.index, C.byref(a), tr._s())
    st.rows += 1


def fit(tr, iterations: int, keep_best: Optional[str] = "mean_return", min_episodes: int = 1, converge=None,
        stop_on_converge: bool = False, poll_every: int = 0) -> TrainingLog:
    """Run `iterations` training iterations, logging each on the device.

    keep_best: the score column ("mean_return", "success_rate", any column before is_best, or
    None); a row is best iff it finished >= min_episodes episodes and its score is strictly above
    every earlier best.  converge: (column, window, threshold) -- converged at the first row
    whose window mean is strictly above the threshold.  With poll_every = k and
    stop_on_converge the header is read every k iterations and the run stops at the first poll
    after convergence; with poll_every = 0 the host reads nothing until the log is first used.
    A second fit on the same trainer continues the same log."""
    if tr.collective:
        raise ValueError("fit() runs on one rank: a collective trainer (world > 1 or a process group) would need "
                         "the ranks' log sums merged between the reduce and the finish stage, which is not built")
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
    st = run_state(tr)
    st.reserve(tr, st.rows + iterations)
    if converge is not None:
        st.window = window
    st.settings = {"keep_best": keep_best, "min_episodes": int(min_episodes),
                   "converge": None if converge is None else [converge[0], window, threshold]}
    for k in range(iterations):
        tr.iteration()
        log_iteration(tr, st, score_col, min_episodes, conv_col, window, threshold)
        if poll_every and stop_on_converge and (k + 1) % int(poll_every) == 0:
            st.host_reads += 1
            if header_dict(st.header.cpu().numpy())["converged_row"] >= 0:
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
    st.host_header.copy_(st.header, non_blocking=True)
    st.event.record(torch.cuda.current_stream(tr.dev))
    log = TrainingLog(window=st.window, settings=st.settings,
                      _pending=(st.event, st.host_table, st.host_header, st.rows))
    st.last_log = weakref.ref(log)
    return log


def best_policy(tr, deterministic: bool = True, seed: Optional[int] = None):
    """The actor of the best logged iteration as a frozen ``MLPActorPolicy``."""
    from .policies import MLPActorPolicy
    st = getattr(tr, "_run", None)
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


def save_checkpoint(tr, path):
    env = tr.env
    st = getattr(tr, "_run", None)
    torch.cuda.synchronize(tr.dev)
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    arrays = {"params": host(tr.params), "m1": host(tr.m1), "m2": host(tr.m2),
              "packed": host(tr.packed.view(torch.int16)), "ep_ret": host(tr.ep_ret),
              "env_state": host(env.state)}
    meta: Dict[str, Any] = {
        "step_count": int(tr.step_count), "iteration_index": int(tr.iteration_index),
        "trainer_config": dataclasses.asdict(tr.cfg),
        "env": env_fingerprint(env), "max_episode_steps": int(env.max_episode_steps),
        "curriculum_configs": [_config_state(c) for c in env.curriculum_configs],
        "scheduler": tr.scheduler.get_state() if tr.scheduler is not None else None,
        "log": None,
    }
    if st is not None:
        arrays.update(log_table=host(st.table[:st.rows]), log_header=host(st.header),
                      best_params=host(st.best_params))
        meta["log"] = {"rows": st.rows, "env_steps": st.env_steps, "window": st.window, "settings": st.settings}
    write_checkpoint(path, arrays, meta)


def load_checkpoint(cls, path, env):
    """A trainer on `env` continuing the checkpointed run.  `env` must have been built with the
    checkpoint's EnvConfig (ValueError otherwise); its state, curriculum table and episode
    limit are overwritten with the checkpoint's."""
    from .experiments import CurriculumConfig, scheduler_from_state
    from .trainer import TrainerConfig
    arrays, meta = read_checkpoint(path)
    want, have = meta["env"], env_fingerprint(env)
    if want != have:
        diff = sorted(k for k in set(want) | set(have) if want.get(k) != have.get(k))
        raise ValueError(f"{path}: the checkpoint was written for another env configuration (differs in "
                         f"{', '.join(diff)})")
    cfg = dict(meta["trainer_config"])
    cfg["betas"] = tuple(cfg["betas"])
    tr = cls(env, TrainerConfig(**cfg))
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
    if meta["log"] is not None:
        lg = meta["log"]
        st = run_state(tr, int(lg["rows"]))
        st.rows, st.env_steps, st.window = int(lg["rows"]), int(lg["env_steps"]), lg["window"]
        st.settings = dict(lg["settings"] or {})
        if st.rows:
            put(st.table[:st.rows], "log_table")
        put(st.header, "log_header")
        put(st.best_params, "best_params")
    torch.cuda.synchronize(dev)
    return tr
