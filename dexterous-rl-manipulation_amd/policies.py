"""Policies -- policies/{simple_learner,random_policy,heuristic_policy}.py.

``SimpleLearner`` keeps the reference surface (``select_action(obs)``,
``update(reward)``, ``reset()``, ``mean_action``, ``best_reward``) and runs its
arithmetic in HIP kernels (``dxrl_learner_select`` / ``dxrl_learner_update``).
Its randomness is the reference's: the process-global legacy ``np.random``
stream (simple_learner.py:60,84), consumed on the host in the same order --
15 normals per action, 15 more only when the reward improves.

``VecSimpleLearner`` is the batched state (N independent learners) that the
fused rollout kernel (``dxrl_rollout_simple``) drives; see training.py.

``MLPActorPolicy`` is the frozen actor of ``PGTrainer`` (no reference
counterpart): the policy object that ``Evaluator`` / ``RobustnessTester`` run
inside the episode-program kernel (``dxrl_evaluate_mlp``), with a host
``select_action`` for the facade path and ``save`` / ``load``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native as N


class VecSimpleLearner:
    """Device state of N SimpleLearners: mean_action f32 [D][N], best f64 [N],
    open-episode return f64 [N], device-RNG counter u64 [N]."""

    def __init__(self, num_envs: int, action_dim: int = 15, learning_rate: float = 0.01,
                 exploration_noise: float = 0.3, action_clip_range: float = 0.5, seed: int = 0, device=None):
        self.device = N.require_gpu(device)
        self.num_envs = int(num_envs)
        self.action_dim = action_dim
        self.learning_rate = learning_rate
        self.exploration_noise = exploration_noise
        self.action_clip_range = action_clip_range
        self.seed = int(seed)
        lay = N.LearnerLayout()
        N.call("dxrl_learner_layout_for", self.num_envs, action_dim, C.byref(lay))
        self.layout = lay
        self._owner, self.state = N.aligned_empty(lay.total_bytes, self.device)
        self.init()

    def _stream(self):
        return N.stream_of(self.device)

    def init(self):
        N.call("dxrl_learner_init", self.device.index, self.num_envs, N.ptr(self.state), self._stream())

    def reset(self, mask: Optional[torch.Tensor] = None):
        N.call("dxrl_learner_reset", self.device.index, self.num_envs, N.ptr(self.state), N.ptr(mask),
               self._stream())

    def native_config(self):
        c = N.LearnerConfig()
        c.learning_rate = float(self.learning_rate)
        c.exploration_noise = float(self.exploration_noise)
        c.action_clip_range = float(self.action_clip_range)
        c.seed = self.seed & (2**64 - 1)
        return c

    def _view(self, off, count, dtype, shape):
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        return self.state[off:off + nbytes].view(dtype).view(*shape)

    @property
    def mean_action(self) -> torch.Tensor:  # [D, N]
        return self._view(self.layout.mean, self.action_dim * self.num_envs, torch.float32,
                          (self.action_dim, self.num_envs))

    @property
    def best_reward(self) -> torch.Tensor:
        return self._view(self.layout.best, self.num_envs, torch.float64, (self.num_envs,))

    @property
    def episode_return(self) -> torch.Tensor:
        return self._view(self.layout.ep_return, self.num_envs, torch.float64, (self.num_envs,))

    def select(self, gauss: torch.Tensor, out: torch.Tensor):
        N.call("dxrl_learner_select", self.device.index, self.num_envs, N.ptr(self.state),
               float(self.exploration_noise), N.ptr(gauss), N.ptr(out), self._stream())
        return out

    def update(self, gauss: torch.Tensor, reward: torch.Tensor, mask: torch.Tensor):
        N.call("dxrl_learner_update", self.device.index, self.num_envs, N.ptr(self.state),
               float(self.learning_rate), float(self.action_clip_range), N.ptr(gauss), N.ptr(reward),
               N.ptr(mask), self._stream())


class SimpleLearner:
    """Drop-in for policies/simple_learner.py:13-99 (one learner)."""

    def __init__(self, action_space, learning_rate: float = 0.01, exploration_noise: float = 0.3,
                 action_clip_range: float = 0.5, device=None):
        self.action_space = action_space
        self.learning_rate = learning_rate
        self.exploration_noise = exploration_noise
        self.action_clip_range = action_clip_range
        d = int(action_space.shape[0])
        self._vec = VecSimpleLearner(1, d, learning_rate, exploration_noise, action_clip_range, device=device)
        self.best_reward = -np.inf
        dev = self._vec.device
        self._g = torch.empty(1, d, dtype=torch.float64, device=dev)
        self._a = torch.empty(1, d, dtype=torch.float32, device=dev)
        self._r = torch.empty(1, dtype=torch.float64, device=dev)
        self._one = torch.ones(1, dtype=torch.uint8, device=dev)

    @property
    def mean_action(self) -> np.ndarray:
        return self._vec.mean_action[:, 0].cpu().numpy()

    def select_action(self, observation: np.ndarray) -> np.ndarray:
        # np.random.normal(0, s, 15) == 0 + s * (15 legacy gauss draws)
        g = np.random.standard_normal(size=self._g.shape[1])
        self._g.copy_(torch.from_numpy(g).view(1, -1))
        self._vec.exploration_noise = self.exploration_noise
        self._vec.select(self._g, self._a)
        return self._a[0].cpu().numpy()

    def update(self, reward: float):
        if reward > self.best_reward:
            g = np.random.standard_normal(size=self._g.shape[1])
            self._g.copy_(torch.from_numpy(g).view(1, -1))
            self._r.fill_(float(reward))
            self._vec.learning_rate = self.learning_rate
            self._vec.action_clip_range = self.action_clip_range
            self._vec.update(self._g, self._r, self._one)
            self.best_reward = reward

    def reset(self):
        self.best_reward = -np.inf


class RandomPolicy:
    """policies/random_policy.py:13-44 -- samples the action space (whose RNG,
    like the reference's, is the Box's own; ``self.rng`` is kept but unused)."""

    def __init__(self, action_space, seed: Optional[int] = None):
        self.action_space = action_space
        self.rng = np.random.default_rng(seed)

    def select_action(self, observation: np.ndarray) -> np.ndarray:
        return self.action_space.sample()

    def reset(self):
        pass


class HeuristicPolicy:
    """policies/heuristic_policy.py:13-68 -- closing motion (-0.5) plus
    f32(U(-0.1, 0.1)) from the global np.random stream, clipped to the space."""

    def __init__(self, action_space, num_fingers: int = 5, joints_per_finger: int = 3):
        self.action_space = action_space
        self.num_fingers = num_fingers
        self.joints_per_finger = joints_per_finger
        self.num_joints = num_fingers * joints_per_finger

    def select_action(self, observation: np.ndarray) -> np.ndarray:
        action = np.full(self.num_joints, -0.5, dtype=np.float32)
        action += np.random.uniform(-0.1, 0.1, size=self.num_joints).astype(np.float32)
        return np.clip(action, self.action_space.low, self.action_space.high)

    def reset(self):
        pass


# csrc/dxrl_pg.h: the actor part of the f32 master parameter block
_OBS_IN, _IN, _H, _HX, _OUT, _ACT = 45, 64, 256, 288, 32, 15
_OFF_W1A, _OFF_W2A, _OFF_W3A = 0, _H * _IN, _H * _IN + _H * _HX
_OFF_LOGSTD = _OFF_W3A + _OUT * _HX
_NPZ_FORMAT = "dxrl-mlp-actor-v1"


def _pcg(seed):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))


def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).float()


class MLPActorPolicy:
    """The frozen MLP(256, 256) actor of ``PGTrainer``: a private f32 copy of the actor blocks of
    the master parameters (``W1a`` [256][64] with the bias in column 45, ``W2a`` [256][288] and
    ``W3a`` [32][288] with the bias in column 256, ``logstd`` [15]), so training on after the
    snapshot does not change it.

    ``deterministic=True``: a = clip(mu(obs), -1, 1), no random draw.  Otherwise
    a = clip(mu(obs) + f32(0 + std g), -1, 1) with std = exp(logstd) (f32, computed once on the
    host) and g from the policy's own ``np.random.Generator(PCG64(seed))`` of standard normals,
    15 per action -- the stream exact-order evaluations consume through a tape; ``seeded(s, n)``
    gives the per-episode streams of the parallel form.

    On the device the policy runs inside ``k_eval_mlp`` (csrc/dxrl_eval_mlp.hip) from the bf16
    pack ``dxrl_pg_pack_weights`` builds on first use.  ``select_action`` is the host form for
    the facade path: the same forward in torch on the CPU with bf16 rounding where the device
    stores bf16 (observation, weights, H1, H2) and f32 accumulation in torch's order."""

    def __init__(self, W1a, W2a, W3a, logstd, deterministic: bool = True, seed: Optional[int] = None):
        f = lambda x, shape: torch.as_tensor(np.array(x, dtype=np.float32, copy=True)).reshape(shape)  # noqa: E731
        self.W1a, self.W2a, self.W3a = f(W1a, (_H, _IN)), f(W2a, (_H, _HX)), f(W3a, (_OUT, _HX))
        self.logstd = f(logstd, (_ACT,))
        self.std = torch.exp(self.logstd)  # f32, once, on the host: the kernel never evaluates exp
        self.deterministic = bool(deterministic)
        self.seed = seed
        self.rng = _pcg(seed)
        from .envs import Box
        self.action_space = Box(low=-1.0, high=1.0, shape=(_ACT,), dtype=np.float32)
        self._w = (_bf16(self.W1a), _bf16(self.W2a[:, :_H]), self.W2a[:, _H].clone(), _bf16(self.W3a[:_ACT, :_H]),
                   self.W3a[:_ACT, _H].clone())
        self._device = {}  # device -> (packed bf16, params f32, std f32)

    @classmethod
    def from_params(cls, params_f32, deterministic: bool = True, seed: Optional[int] = None) -> "MLPActorPolicy":
        """From a master-layout parameter tensor (``PGTrainer.params``; the critic part is not read)."""
        p = params_f32.detach().float().cpu().numpy() if isinstance(params_f32, torch.Tensor) \
            else np.asarray(params_f32, np.float32)
        if p.ndim != 1 or p.size < _OFF_LOGSTD + _ACT:
            raise ValueError("params must be the flat f32 master parameter block")
        return cls(p[_OFF_W1A:_OFF_W2A], p[_OFF_W2A:_OFF_W3A], p[_OFF_W3A:_OFF_LOGSTD],
                   p[_OFF_LOGSTD:_OFF_LOGSTD + _ACT], deterministic, seed)

    # ------------------------------------------------------------------ host form
    def mean_action_of(self, observation) -> torch.Tensor:
        """mu [15] (f32) of one observation."""
        W1, W2, b2, W3, b3 = self._w
        x = torch.zeros(_IN)
        x[:_OBS_IN] = _bf16(torch.as_tensor(np.asarray(observation, dtype=np.float32)).reshape(_OBS_IN))
        x[_OBS_IN] = 1.0
        h1 = _bf16(torch.tanh(x[None] @ W1.T))
        h2 = _bf16(torch.tanh(h1 @ W2.T + b2))
        return (h2 @ W3.T + b3)[0]

    def select_action(self, observation: np.ndarray) -> np.ndarray:
        mu = self.mean_action_of(observation).numpy()
        if not self.deterministic:
            g = self.rng.standard_normal(_ACT)
            mu = mu + (0.0 + self.std.numpy().astype(np.float64) * g).astype(np.float32)
        return np.clip(mu, np.float32(-1.0), np.float32(1.0)).astype(np.float32)

    def reset(self):
        pass

    def seeded(self, seed, n: int) -> np.ndarray:
        """A fresh per-episode stream: n standard normals of PCG64(seed)."""
        return _pcg(int(seed)).standard_normal(n)

    # ------------------------------------------------------------------ device form
    def master_params(self) -> np.ndarray:
        """The actor blocks in a zeroed master-layout block (critic part zero)."""
        p_, b_ = C.c_int64(), C.c_int64()
        N.call("dxrl_pg_sizes", C.byref(p_), C.byref(b_))
        p = np.zeros(p_.value, np.float32)
        p[_OFF_W1A:_OFF_W2A] = self.W1a.numpy().ravel()
        p[_OFF_W2A:_OFF_W3A] = self.W2a.numpy().ravel()
        p[_OFF_W3A:_OFF_LOGSTD] = self.W3a.numpy().ravel()
        p[_OFF_LOGSTD:_OFF_LOGSTD + _ACT] = self.logstd.numpy()
        return p

    def device_tensors(self, device):
        """(bf16 pack, f32 master, f32 std [15]) on ``device``, built on first use."""
        dev = N.require_gpu(device)
        if dev not in self._device:
            p_, b_ = C.c_int64(), C.c_int64()
            N.call("dxrl_pg_sizes", C.byref(p_), C.byref(b_))
            params = torch.from_numpy(self.master_params()).to(dev)
            packed = torch.zeros(b_.value, dtype=torch.bfloat16, device=dev)
            with torch.cuda.device(dev):
                N.call("dxrl_pg_pack_weights", dev.index, N.ptr(params), N.ptr(packed), N.stream_of(dev))
            self._device[dev] = (packed, params, self.std.to(dev))
        return self._device[dev]

    # ------------------------------------------------------------------ files
    def save(self, path):
        """One .npz: the four f32 blocks, the mode flag and a format tag."""
        with open(path, "wb") as f:
            np.savez(f, format=np.array(_NPZ_FORMAT), W1a=self.W1a.numpy(), W2a=self.W2a.numpy(),
                     W3a=self.W3a.numpy(), logstd=self.logstd.numpy(), deterministic=np.array(self.deterministic))

    @classmethod
    def load(cls, path, seed: Optional[int] = None) -> "MLPActorPolicy":
        with np.load(path, allow_pickle=False) as z:
            if str(z["format"]) != _NPZ_FORMAT:
                raise ValueError(f"{path}: not a {_NPZ_FORMAT} file")
            return cls(z["W1a"], z["W2a"], z["W3a"], z["logstd"], bool(z["deterministic"]), seed)
