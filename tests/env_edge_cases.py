"""Crafted env states that reach the rare branches of the env step (test infrastructure).

The env physics runs in four device forms (csrc/dxrl_device.h env_step and the lane-split forms
in dxrl_pg_rollout16.hip, dxrl_pg_rollout8.hip and dxrl_eval_row.h, which k_eval_ls and k_eval_mlp
share), all built from the formulas that dxrl_device.h states once.
States that come from ordinary resets and ordinary policies never take the x / y wall stops, the
z ceiling, the joint clip at +-1, sqrt_below()'s exact-root branch, most of the 32 x 33 contact /
previous-contact combinations, or the truncation bound.  ``build(mode)`` returns lanes that do, in
pure NumPy plus the pinned CPU oracle:

* ``mode="state"``: the full env state (for kernels that read the state slab: dxrl_env_step and
  the three policy-gradient rollout kernels);
* ``mode="reset"``: states reachable through a reset (zero velocities, step count 0, no previous
  contacts, f32 object position) given as the 21 reset draws -- for dxrl_env_reset and the
  evaluation kernels, whose episodes start from a reset tape.

``check(cases)`` runs the oracle over every lane and asserts, from the oracle's own state, that
each lane meets its named edge at its named step, that every cell of every family is present and
that no episode ends before its edge.  The GPU tests run it before they trust the lanes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from oracle.dx_oracle import HI, LO, OracleCurriculum, OracleEnv

f32 = np.float32
D, F, J = 15, 5, 3
T = 4                       # steps of the action table
MAX_EPISODE_STEPS = 200     # the env's truncation bound the lanes are built for
PG_MAX_STEPS = 150          # TrainerConfig.max_steps the rollout-bound lanes are built for

# flag word bits (csrc/dxrl_device.h)
PREV_SHIFT, HAS_PREV, OP_IS_F32, HAS_OBJECT, FRIC_F64 = 8, 1 << 16, 1 << 17, 1 << 18, 1 << 19

FAR_SIZE = 0.05
KNIFE_ULPS = (-2, -1, 0, 1, 2)
KNIFE_WHEN_STATE = ("post0", "post2")
KNIFE_WHEN_RESET = ("reset", "post0", "post1")
BAND = 2.0 ** -40           # sqrt_below()'s slow-path band, relative to the squared threshold

_ONE = f32(1.0)
# every special value the action clip sees (NaN stays out: the oracle's min and np.min differ on it)
SPECIAL_ACTIONS = np.array(
    [np.inf, -np.inf, 1.0, -1.0, np.nextafter(_ONE, f32(0)), np.nextafter(-_ONE, f32(0)),
     np.nextafter(_ONE, f32(2)), np.nextafter(-_ONE, f32(-2)), -0.0, 1e-45, -1e-45, 1e-39, -1e-39,
     1e30, -1e30], dtype=np.float32)
assert SPECIAL_ACTIONS.size == D


@dataclass
class Lane:
    family: str
    cell: Tuple                       # the cell of its family this lane fills
    step: int                         # the step at which its edge occurs (-1: at the reset itself)
    jp: np.ndarray                    # f32 [15]
    jv: np.ndarray                    # f32 [15]
    op: np.ndarray                    # f64 [3]
    ov: np.ndarray                    # f32 [3]
    size: float
    actions: np.ndarray               # f32 [T][15]
    op_is_f32: bool = True
    prev: Optional[int] = None        # previous contact mask, None = no previous contacts
    fric_f64: bool = False
    t: int = 0
    mass: float = 0.1
    fric: float = 0.5
    contacts: int = 0                 # contact mask of the state itself (filled by build)

    @property
    def name(self) -> str:
        return self.family + "/" + "/".join(str(c) for c in self.cell)


@dataclass
class Cases:
    mode: str
    lanes: List[Lane]
    max_episode_steps: int = MAX_EPISODE_STEPS
    pg_max_steps: int = PG_MAX_STEPS

    def __len__(self):
        return len(self.lanes)

    def names(self):
        return [ln.name for ln in self.lanes]

    def stack(self, attr, dtype):
        return np.stack([np.asarray(getattr(ln, attr), dtype) for ln in self.lanes])

    def actions(self) -> np.ndarray:
        """f32 [T][L][15]"""
        return np.ascontiguousarray(np.stack([ln.actions for ln in self.lanes], axis=1), np.float32)

    def flags(self) -> np.ndarray:
        out = np.zeros(len(self.lanes), np.uint32)
        for i, ln in enumerate(self.lanes):
            w = ln.contacts | HAS_OBJECT
            if ln.prev is not None:
                w |= HAS_PREV | (ln.prev << PREV_SHIFT)
            if ln.op_is_f32:
                w |= OP_IS_F32
            if ln.fric_f64:
                w |= FRIC_F64
            out[i] = w
        return out

    def reset_draws(self) -> np.ndarray:
        """f64 [L][21]: joints, size, mass, friction, spawn (mode "reset")."""
        assert self.mode == "reset"
        d = np.empty((len(self.lanes), D + 6))
        for i, ln in enumerate(self.lanes):
            d[i, :D] = ln.jp.astype(np.float64)
            d[i, D:D + 3] = ln.size, ln.mass, ln.fric
            d[i, D + 3:] = ln.op
        return d

    def rows(self) -> np.ndarray:
        """Curriculum row per lane (mode "reset"): 0 = Python-float friction, 1 = numpy.float64."""
        return np.array([int(ln.fric_f64) for ln in self.lanes], np.int32)


def reset_curricula():
    """(kwargs for CurriculumConfig, OracleCurriculum) of the two rows ``Cases.rows`` indexes: the
    size is drawn (slot 15 of the reset draws), mass and friction are the row's constants."""
    out = []
    for f64 in (False, True):
        kw = dict(object_size=FAR_SIZE, object_mass=0.1, friction_coefficient=np.float64(0.5) if f64 else 0.5,
                  object_size_range=(0.0, 4.0))
        out.append((kw, OracleCurriculum(object_size=FAR_SIZE, object_mass=0.1, friction_coefficient=0.5,
                                         size_range=(0.0, 4.0), friction_is_np_float64=f64)))
    return out


# ------------------------------------------------------------------ oracle
def oracle_of(cases: Cases, i: int, dense: bool = True, max_episode_steps: Optional[int] = None) -> OracleEnv:
    """The oracle env of lane i, in the lane's initial state."""
    ln = cases.lanes[i]
    mes = cases.max_episode_steps if max_episode_steps is None else max_episode_steps
    if cases.mode == "reset":
        o = OracleEnv(cur=reset_curricula()[int(ln.fric_f64)][1], dense=dense, max_episode_steps=mes)
        o.reset(cases_draw(ln))
        return o
    cur = OracleCurriculum(object_size=ln.size, object_mass=ln.mass, friction_coefficient=ln.fric,
                           friction_is_np_float64=ln.fric_f64)
    o = OracleEnv(cur=cur, dense=dense, max_episode_steps=mes)
    o.jp, o.jv = [f32(x) for x in ln.jp], [f32(x) for x in ln.jv]
    o.op, o.ov = [float(x) for x in ln.op], [f32(x) for x in ln.ov]
    o.op_is_f32 = ln.op_is_f32
    o.size, o.mass, o.fric = float(ln.size), float(ln.mass), float(ln.fric)
    o.t = int(ln.t)
    o._contacts()
    o.prev = None if ln.prev is None else [(ln.prev >> f) & 1 for f in range(F)]
    return o


def cases_draw(ln: Lane) -> np.ndarray:
    d = np.empty(D + 6)
    d[:D] = ln.jp.astype(np.float64)
    d[D:D + 3] = ln.size, ln.mass, ln.fric
    d[D + 3:] = ln.op
    return d


def mask_of(contacts) -> int:
    return sum(int(c) << f for f, c in enumerate(contacts))


def snap(o: OracleEnv, **kw):
    s = dict(dist=list(o.dist), tips=list(o.tips), thr=o.size * 1.5, mask=mask_of(o.contacts), op=list(o.op),
             ov=[f32(v) for v in o.ov], jp=[f32(v) for v in o.jp], jv=[f32(v) for v in o.jv], t=o.t)
    s.update(kw)
    return s


def trace(cases: Cases, i: int):
    """Oracle states of lane i: entry -1 the initial state, entries 0..T-1 after each step of the
    lane's action table (stepping on past an episode end, as dxrl_env_step does)."""
    o = oracle_of(cases, i)
    ln = cases.lanes[i]
    out = {-1: snap(o, term=False, trunc=False, prev=None, obs=o.obs())}
    for s in range(T):
        prev = None if o.prev is None else mask_of(o.prev)
        ob, r, te, tr = o.step(ln.actions[s])
        out[s] = snap(o, term=te, trunc=tr, prev=prev, obs=ob, reward=r)
    return out


# ------------------------------------------------------------------ builders
def _rng(*key: int):
    return np.random.default_rng(list(key))


def _zero_actions():
    return np.zeros((T, D), np.float32)


def _far_lane(family, cell, step, **kw) -> Lane:
    """Joints at zero, the object far from every tip (no contacts), nothing moving."""
    base = dict(jp=np.zeros(D, np.float32), jv=np.zeros(D, np.float32), op=np.array([0.15, -0.15, 0.25]),
                ov=np.zeros(3, np.float32), size=FAR_SIZE, actions=_zero_actions())
    base.update(kw)
    base["op"] = np.asarray(base["op"], np.float64)
    if base.get("op_is_f32", True):
        base["op"] = base["op"].astype(np.float32).astype(np.float64)
    return Lane(family, cell, step, **base)


def ulps(x: float, k: int) -> float:
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def _knife(mode: str) -> List[Lane]:
    """Finger f's distance within a few ulps of 1.5 size: every such lane is inside sqrt_below()'s
    2^-40 band, so the lane-split kernels take the exact-root branch."""
    lanes = []
    whens = KNIFE_WHEN_STATE if mode == "state" else KNIFE_WHEN_RESET
    for when in whens:
        step = -1 if when == "reset" else int(when[4:])
        for f in range(F):
            for k in KNIFE_ULPS:
                rng = _rng(7, len(lanes))
                jp = (-0.95 + rng.uniform(-0.04, 0.04, D)).astype(np.float32)  # the other tips: far away
                jp[J * f:J * f + J] = rng.uniform(-0.1, 0.1, J).astype(np.float32)
                op = np.array([rng.uniform(0.05, 0.1), rng.uniform(0.05, 0.1), rng.uniform(0.05, 0.2)])
                op = op.astype(np.float32).astype(np.float64)
                st = mode == "state"
                ln = Lane("knife", (when, f, k), step, jp=jp,
                          jv=(rng.uniform(-0.05, 0.05, D).astype(np.float32) if st else np.zeros(D, np.float32)),
                          op=op, ov=(np.array([0.0, 0.0, -0.2], np.float32) if st else np.zeros(3, np.float32)),
                          size=FAR_SIZE, actions=rng.uniform(-1.3, 1.3, (T, D)).astype(np.float32),
                          prev=(0 if st and k % 2 else None), fric_f64=bool(f % 2))
                probe = Cases(mode, [ln])
                d = trace(probe, 0)[step]["dist"][f]   # the distance does not depend on the size
                ln.size = ulps(d / 1.5, k)
                lanes.append(ln)
    # d == 0 (a tip on the object), size == 0, a size that makes all five fingers touch
    for f in range(F):
        jp = np.full(D, -1.0, np.float32)
        jp[J * f:J * f + J] = 0.0
        for cell, size in (("zero_dist", FAR_SIZE), ("zero_size", 0.0)):
            lanes.append(Lane("knife", (cell, f), 0, jp=jp.copy(), jv=np.zeros(D, np.float32), op=np.zeros(3),
                              ov=np.zeros(3, np.float32), size=size, actions=_zero_actions()))
    lanes.append(_far_lane("knife", ("all_five",), 0, size=1.0))
    return lanes


def _mask_geometry(cur: int):
    c = 0.1
    jp = np.full(D, -1.0, np.float32)                       # joint sum -3: tip at -0.3
    for f in range(F):
        if (cur >> f) & 1:
            jp[J * f:J * f + J] = (0.4, 0.3, 0.3)           # joint sum 10 c: tip on the object
    return jp, np.full(3, float(f32(c)))


def _mask_grid(mode: str) -> List[Lane]:
    """Every contact mask against no previous mask and (mode "state") every previous mask."""
    lanes = []
    for cur in range(32):
        for prev in ([-1] + list(range(32)) if mode == "state" else [-1]):
            jp, op = _mask_geometry(cur)
            lanes.append(Lane("mask", (cur, prev), 0, jp=jp, jv=np.zeros(D, np.float32), op=op,
                              ov=np.zeros(3, np.float32), size=FAR_SIZE, actions=_zero_actions(),
                              prev=None if prev < 0 else prev))
    return lanes


def joint_update(jp, jv, a):
    """One joint's ME:203-207 in f32: (new velocity, unclipped new position)."""
    a = f32(min(max(f32(a), f32(-1)), f32(1)))
    v = f32(f32(f32(0.9) * f32(jv)) + f32(f32(0.1) * a))
    return v, f32(f32(jp) + f32(v * f32(0.01)))


def _joint_limits(mode: str) -> List[Lane]:
    lanes = []
    for j in range(D):
        for bound in (-1.0, 1.0):
            jv0 = f32(0.5 * bound) if mode == "state" else f32(0.0)
            v, _ = joint_update(0.0, jv0, bound)
            inc = f32(v * f32(0.01))
            for kind in ("cross", "land", "inside"):
                if kind == "cross":
                    p0 = f32(bound - float(inc) / 2)
                elif kind == "inside":
                    p0 = f32(bound * 0.99)
                else:
                    p0 = f32(bound - float(inc))
                    for _ in range(8):  # a start from which the f32 sum lands exactly on the bound
                        if joint_update(p0, jv0, bound)[1] == f32(bound):
                            break
                        p0 = np.nextafter(p0, f32(bound))
                jp, jv = np.zeros(D, np.float32), np.zeros(D, np.float32)
                jp[j], jv[j] = p0, jv0
                act = _zero_actions()
                act[:, j] = bound
                lanes.append(_far_lane("joint", (j, int(bound), kind), 0, jp=jp, jv=jv, actions=act,
                                       op=np.array([-0.2 * bound, -0.2 * bound, 0.3])))
    return lanes


def wall_cells(mode: str):
    """(axis, side, velocity, landing) cells.  Left out because the physics cannot produce them:
    on z gravity adds -0.0981 to the velocity every step, so the velocity never stays zero and a
    velocity away from a z wall always leaves it."""
    cells = []
    if mode == "state":
        for axis in (0, 1):
            for side in ("lo", "hi"):
                for vel in ("into", "away", "zero"):
                    for land in ("on", "short"):
                        cells.append((axis, side, vel, land))
        cells += [(2, "lo", "into", "on"), (2, "lo", "into", "short"), (2, "lo", "away", "short"),
                  (2, "hi", "into", "on"), (2, "hi", "into", "short"), (2, "hi", "away", "short")]
    else:  # velocities are zero after a reset: only gravity acts
        cells += [(2, "lo", "into", "on"), (2, "lo", "into", "short"), (2, "hi", "away", "short")]
    return cells


def _walls(mode: str) -> List[Lane]:
    lanes = []
    for axis, side, vel, land in wall_cells(mode):
        bound = (LO if side == "lo" else HI)[axis]
        sign = -1.0 if side == "lo" else 1.0
        if axis < 2:
            v0 = {"into": 0.5 * sign, "away": -0.5 * sign, "zero": 0.0}[vel]
            if vel == "away" and land == "on":
                v0 = -1e-30 * sign                  # the position increment is absorbed: it stays on the wall
            p0 = {("into", "on"): bound - 0.001 * sign, ("into", "short"): bound - 0.05 * sign,
                  ("away", "on"): bound, ("away", "short"): bound, ("zero", "on"): bound,
                  ("zero", "short"): 0.0}[(vel, land)]
        elif side == "lo":
            v0 = 0.5 if vel == "away" else 0.0
            p0 = {"on": 0.0005, "short": 0.1}[land] if vel == "into" else 0.0
        else:
            v0 = 0.5 if vel == "into" else 0.0       # into the ceiling: more than one step of gravity
            p0 = {"on": 0.2995, "short": 0.2}[land] if vel == "into" else 0.3
        for op32 in ((True, False) if mode == "state" else (True,)):
            for f64 in (False, True):
                op = np.array([0.15, -0.15, 0.25])
                ov = np.zeros(3, np.float32)
                op[axis], ov[axis] = p0, v0
                lanes.append(_far_lane("wall", (axis, side, vel, land, int(op32), int(f64)), 0, op=op, ov=ov,
                                       op_is_f32=op32, fric_f64=f64, jp=np.full(D, -0.5, np.float32)))
    # an object placed beyond a wall (a spawn range wider than the workspace): clipped at step 0
    for axis in range(3):
        for side in ("lo", "hi"):
            sign = -1.0 if side == "lo" else 1.0
            op = np.array([0.15, -0.15, 0.25])
            op[axis] = (LO if side == "lo" else HI)[axis] + 0.3 * sign
            lanes.append(_far_lane("wall", ("beyond", axis, side), 0, op=op, jp=np.full(D, -0.5, np.float32),
                                   fric_f64=bool(axis % 2)))
    return lanes


def object_velocity_before_stop(ln: Lane, axis: int):
    """ME:215-219 for one axis from the lane's initial state: the velocity the wall test sees."""
    damp = 1.0 - (ln.fric * 0.1 * 0.01)
    v = f32(float(ln.ov[axis]) * damp) if ln.fric_f64 else f32(f32(ln.ov[axis]) * f32(damp))
    return f32(float(v) + (0.0, 0.0, -9.81 * 0.01)[axis])


def _truncation(cases_mes: int, pg_ms: int) -> List[Lane]:
    lanes = []
    for which, bound in (("episode", cases_mes), ("rollout", pg_ms)):
        for delta in (2, 1, 0):
            lanes.append(_far_lane("trunc", (which, delta), delta if which == "episode" else max(delta - 1, 0),
                                   t=bound - delta, prev=0))
    return lanes


def _special_actions() -> List[Lane]:
    lanes = []
    for rot in range(D):
        act = np.stack([np.roll(SPECIAL_ACTIONS, rot + s) for s in range(T)]).astype(np.float32)
        lanes.append(_far_lane("action", (rot,), 0, actions=act, jp=np.full(D, 0.05, np.float32)))
    return lanes


def _pad(mode: str, k: int) -> Lane:
    rng = _rng(99, k)
    st = mode == "state"
    return _far_lane("pad", (k,), 0, jp=rng.uniform(-0.1, 0.1, D).astype(np.float32),
                     jv=(rng.uniform(-0.05, 0.05, D).astype(np.float32) if st else np.zeros(D, np.float32)),
                     actions=rng.uniform(-1.3, 1.3, (T, D)).astype(np.float32))


FAMILIES = ("knife", "mask", "joint", "wall", "trunc", "action")


def build(mode: str = "state", families=FAMILIES) -> Cases:
    """The lanes of every family in ``families`` (all of them by default), padded with ordinary
    lanes until the lane count is 8 modulo 16: no multiple of 16, 32 or 256 (ragged last rows,
    waves and workgroups), yet lanes x T a multiple of 32, which PGTrainer requires of its tape."""
    assert mode in ("state", "reset")
    lanes: List[Lane] = []
    if "knife" in families:
        lanes += _knife(mode)
    if "mask" in families:
        lanes += _mask_grid(mode)
    if "joint" in families:
        lanes += _joint_limits(mode)
    if "wall" in families:
        lanes += _walls(mode)
    if "trunc" in families and mode == "state":
        lanes += _truncation(MAX_EPISODE_STEPS, PG_MAX_STEPS)
    if "action" in families:
        lanes += _special_actions()
    k = 0
    while k < 3 or len(lanes) % 16 != 8:
        lanes.append(_pad(mode, k))
        k += 1
    cases = Cases(mode, lanes)
    for i, ln in enumerate(lanes):  # the contact bits of the state itself (observation row 0 shows them)
        if mode == "state":
            ln.contacts = mask_of(oracle_of(cases, i).contacts)
    return cases


# ------------------------------------------------------------------ the checker
def expected_cells(mode: str):
    """Every cell each family must hold."""
    cells = set()
    whens = KNIFE_WHEN_STATE if mode == "state" else KNIFE_WHEN_RESET
    cells |= {("knife", (w, f, k)) for w in whens for f in range(F) for k in KNIFE_ULPS}
    cells |= {("knife", (c, f)) for c in ("zero_dist", "zero_size") for f in range(F)} | {("knife", ("all_five",))}
    prevs = [-1] + list(range(32)) if mode == "state" else [-1]
    cells |= {("mask", (c, p)) for c in range(32) for p in prevs}
    cells |= {("joint", (j, b, k)) for j in range(D) for b in (-1, 1) for k in ("cross", "land", "inside")}
    op32s = (1, 0) if mode == "state" else (1,)
    cells |= {("wall", c + (o, g)) for c in wall_cells(mode) for o in op32s for g in (0, 1)}
    cells |= {("wall", ("beyond", a, s)) for a in range(3) for s in ("lo", "hi")}
    if mode == "state":
        cells |= {("trunc", (w, d)) for w in ("episode", "rollout") for d in (2, 1, 0)}
    cells |= {("action", (r,)) for r in range(D)}
    return cells


def in_band(s, f):
    dx, dy, dz = (s["tips"][f] - s["op"][k] for k in range(3))
    x, q = (dx * dx + dy * dy) + dz * dz, s["thr"] * s["thr"]
    return q * (1.0 - BAND) <= x <= q * (1.0 + BAND)


def check(cases: Cases, traces=None):
    """Assert from the oracle's own state that every lane meets its named edge at its named step,
    that every cell of every family is present, and that no episode ends before its edge.
    Returns the oracle traces (lane -> {step -> state}) for the callers that compare against them."""
    mode, L = cases.mode, len(cases)
    assert L % 16 == 8 and L % 32 and L % 256 and (L * T) % 32 == 0
    have = {(ln.family, ln.cell) for ln in cases.lanes if ln.family != "pad"}
    missing = expected_cells(mode) - have
    assert not missing, f"cells missing from the builder: {sorted(missing, key=str)[:8]} ({len(missing)})"
    assert len(have) == sum(ln.family != "pad" for ln in cases.lanes), "a cell is filled twice"
    traces = traces or {i: trace(cases, i) for i in range(L)}
    relations = {w: set() for w in (KNIFE_WHEN_STATE if mode == "state" else KNIFE_WHEN_RESET)}
    seen_actions = set()
    for i, ln in enumerate(cases.lanes):
        tr, c, name = traces[i], ln.cell, ln.name
        for s in range(ln.step):
            assert not (tr[s]["term"] or tr[s]["trunc"]), f"{name}: the episode ends at step {s}, before its edge"
        e = tr[ln.step]
        if ln.family == "knife" and len(c) == 3:
            when, f, _ = c
            assert in_band(e, f), f"{name}: outside sqrt_below's slow-path band"
            d, thr = e["dist"][f], e["thr"]
            assert ((e["mask"] >> f) & 1) == int(d < thr), name
            relations[when].add("lt" if d < thr else ("eq" if d == thr else "gt"))
        elif ln.family == "knife" and c[0] in ("zero_dist", "zero_size"):
            f = c[1]
            for s in (-1, 0):
                assert tr[s]["dist"][f] == 0.0, name
                assert tr[s]["mask"] == ((1 << f) if c[0] == "zero_dist" else 0), name
            assert (e["thr"] == 0.0) == (c[0] == "zero_size"), name
        elif ln.family == "knife":
            assert tr[-1]["mask"] == 31 and e["mask"] == 31 and e["term"], name
        elif ln.family == "mask":
            cur, prev = c
            assert e["mask"] == cur and tr[-1]["mask"] == cur, name
            assert e["prev"] == (None if prev < 0 else prev), name
            assert e["term"] == (bin(cur).count("1") >= 3), name
            assert tr[1]["prev"] == cur and tr[1]["mask"] == cur, name   # the next step: unchanged contacts
        elif ln.family == "joint":
            j, bound, kind = c
            v, un = joint_update(tr[-1]["jp"][j], tr[-1]["jv"][j], ln.actions[0][j])
            assert v == e["jv"][j], name
            if kind == "cross":
                assert abs(un) > 1.0 and np.sign(un) == bound and e["jp"][j] == f32(bound), name
            elif kind == "land":
                assert un == f32(bound) and e["jp"][j] == f32(bound), name
            else:
                assert abs(un) < 1.0 and e["jp"][j] == un, name
            assert e["mask"] == 0, name
        elif ln.family == "wall" and c[0] == "beyond":
            _, axis, side = c
            bound = (LO if side == "lo" else HI)[axis]
            p0 = tr[-1]["op"][axis]
            assert (p0 < bound) if side == "lo" else (p0 > bound), name
            assert e["op"][axis] == bound and e["mask"] == 0, name
        elif ln.family == "wall":
            axis, side, vel, land, op32, f64 = c
            bound = (LO if side == "lo" else HI)[axis]
            sign = -1.0 if side == "lo" else 1.0
            vpre = object_velocity_before_stop(ln, axis)
            p, v = e["op"][axis], e["ov"][axis]
            assert ln.op_is_f32 == bool(op32) and ln.fric_f64 == bool(f64), name
            assert (p == bound) if land == "on" else (LO[axis] < p < HI[axis]), (name, p)
            if vel == "zero":
                assert vpre == 0.0 and v == 0.0, name
            elif vel == "into":
                assert vpre != 0.0 and np.sign(vpre) == sign, name
                assert v == (f32(0.0) if land == "on" else vpre), name   # stopped on the wall only
            else:
                assert vpre != 0.0 and np.sign(vpre) == -sign and v == vpre, name  # never stopped
            assert e["mask"] == 0, name
        elif ln.family == "trunc":
            which, delta = c
            bound = cases.max_episode_steps if which == "episode" else cases.pg_max_steps
            assert ln.t == bound - delta, name
            for s in range(T):
                assert not tr[s]["term"], name
                if which == "episode":
                    assert tr[s]["trunc"] == (s >= delta), (name, s)
                else:  # the rollout's own bound: step count after the step >= max_steps
                    assert (tr[s]["t"] >= bound) == (s >= ln.step) and not tr[s]["trunc"], (name, s)
        elif ln.family == "action":
            seen_actions |= {(k, float(a).hex()) for k, a in enumerate(ln.actions[0])}
            for s in range(T):
                assert sorted(ln.actions[s].tolist()) == sorted(SPECIAL_ACTIONS.tolist()), name
                assert all(abs(p) <= 1.0 for p in tr[s]["jp"]), name
    for when, rel in relations.items():
        assert rel == {"lt", "eq", "gt"}, f"knife/{when}: only {sorted(rel)} of lt / eq / gt occur"
    assert seen_actions == {(k, float(a).hex()) for k in range(D) for a in SPECIAL_ACTIONS}
    return traces
