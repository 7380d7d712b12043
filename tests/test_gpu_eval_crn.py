"""GPU: the stream period of the MLP episode kernel (dxrl_eval_args.stream_period,
csrc/dxrl_eval_mlp.hip) -- common random numbers across the levels of a level-major launch.

test_gpu_eval_mlp.py's parameters and configs, trajectories kept.  Launches are level-major:
level l, object o, episode k is lane, segment and record (l G + o) K + k with G = 3 objects x
K = 5 episodes, so P = 15 and a 16-row workgroup holds rows of two levels; max_steps 12.  Every
case runs with a deterministic and with a stochastic actor.

With stream_period = 15 the three device keys are taken from the index modulo 15: every level's
slice is, bit for bit, the 15-lane launch of that level alone, the repeated baseline equals the
first, a noisy level starts from the baseline's spawn, and two observation-noise levels whose
stds are powers of two apart carry the same standard normals (the scaling is exact, only the
additions round: per element |(v_c - v_0) - 4 (v_b - v_0)| <= 2^-24 (|v_c| + 4 |v_b|))."""
import ctypes as C

import numpy as np
import pytest
import torch

import dexterous_rl_manipulation_amd as pkg
from dexterous_rl_manipulation_amd import _native as N
from dexterous_rl_manipulation_amd import evaluator as evr

import eval_mlp_reference as E
from test_eval_host import cfg_of
from test_gpu_eval_mlp import PARAMS, assert_same_records

pytestmark = pytest.mark.gpu

LEVELS = [(0.0, 0.0), (0.03125, 0.0), (0.125, 0.0), (0.0, 0.05), (0.125, 0.05), (0.0, 0.0)]
G, K, MAX_STEPS, SEED = 3, 5, 12, 21
P = G * K
BASE, OBS_B, OBS_C, DYN, LAST = 0, 1, 2, 3, 5


def configs():
    return [cfg_of("variable"), cfg_of("medium"), cfg_of("easy")]


def program(levels, lanes=None):
    """The level-major plan of `levels` (its first `lanes` lanes)."""
    p = evr.EpisodeProgram(configs(), "dense", max_episode_steps=50, max_steps=MAX_STEPS)
    todo = [(obs, dyn, o, k) for obs, dyn in levels for o in range(G) for k in range(K)]
    for obs, dyn, o, k in todo[:lanes]:
        p.add_lane([evr.Segment(o, [k], obs, dyn, noise_seed=(0, k))])
    return p


def rows(level):
    return np.arange(level * P, (level + 1) * P)


class Runs:
    def __init__(self, stochastic):
        self.prog = evr.policy_program(E.policy_of(PARAMS, deterministic=not stochastic, seed=1))
        kw = self.kw = dict(host_resets=False, host_noise=False, device_seed=SEED, trajectories=True)
        self.crn = program(LEVELS).run(self.prog, stream_period=P, **kw)
        self.plain = program(LEVELS).run(self.prog, **kw)
        self.alone = [program([lv]).run(self.prog, **kw) for lv in LEVELS]
        self.ragged = program(LEVELS, lanes=40).run(self.prog, stream_period=P, **kw)


@pytest.fixture(scope="module", params=[False, True], ids=["deterministic", "stochastic"])
def runs(request):
    r = Runs(request.param)
    r.stochastic = request.param
    return r


def test_every_level_slice_is_that_level_launched_alone(runs):
    assert len(runs.crn.ep_length) == len(LEVELS) * P
    for l in range(len(LEVELS)):
        assert_same_records(runs.crn, runs.alone[l], rows(l), np.arange(P), used=False)
        assert np.array_equal(runs.crn.policy_used[rows(l)], runs.alone[l].policy_used), l
    assert runs.crn.ep_length.min() >= 1 and runs.crn.ep_length.max() <= MAX_STEPS


def test_the_baseline_is_unchanged_and_repeats(runs):
    assert_same_records(runs.crn, runs.crn, rows(BASE), rows(LAST), used=False)
    assert_same_records(runs.crn, runs.plain, rows(BASE), rows(BASE), used=False)


def test_without_a_period_the_levels_draw_their_own_episodes(runs):
    a, b = runs.plain.obs_traj[rows(BASE), 0], runs.plain.obs_traj[rows(LAST), 0]
    assert not np.array_equal(a, b)
    assert not np.array_equal(runs.plain.ep_return[rows(BASE)], runs.plain.ep_return[rows(LAST)])


def test_a_noisy_level_starts_from_the_baseline_spawn(runs):
    r = runs.crn
    assert np.array_equal(r.obs_traj[rows(DYN), 0], r.obs_traj[rows(BASE), 0])
    if not runs.stochastic:  # the same observation through the same actor, before any dynamics noise
        assert np.array_equal(r.act_traj[rows(DYN), 0], r.act_traj[rows(BASE), 0])
    # the level is noisy all the same: dynamics noise moves the later observations
    assert not np.array_equal(r.obs_traj[rows(DYN), 1], r.obs_traj[rows(BASE), 1])
    # and without the period the level's spawns are its own
    assert not np.array_equal(runs.plain.obs_traj[rows(DYN), 0], runs.plain.obs_traj[rows(BASE), 0])


def test_observation_noise_levels_share_their_standard_normals(runs):
    r = runs.crn
    v0, vb, vc = (r.obs_traj[rows(l), 0].astype(np.float64) for l in (BASE, OBS_B, OBS_C))
    assert np.count_nonzero(vb != v0) > 0.9 * v0.size  # the noise is there
    err = np.abs((vc - v0) - 4.0 * (vb - v0))
    bound = 2.0 ** -24 * (np.abs(vc) + 4.0 * np.abs(vb))
    print("max err / bound", float((err / np.maximum(bound, 1e-300)).max()), "max err", float(err.max()))
    assert np.all(err <= bound)
    # keyed by record index, the two levels' normals are unrelated
    p0, pb, pc = (runs.plain.obs_traj[rows(l), 0].astype(np.float64) for l in (BASE, OBS_B, OBS_C))
    assert not np.all(np.abs((pc - p0) - 4.0 * (pb - p0)) <= 2.0 ** -24 * (np.abs(pc) + 4.0 * np.abs(pb)))


def test_a_lane_count_that_is_no_multiple_of_the_period(runs):
    idx = np.arange(40)
    assert_same_records(runs.ragged, runs.crn, idx, idx, used=False)
    assert np.array_equal(runs.ragged.policy_used, runs.crn.policy_used[:40])


def test_refusals_before_any_launch():
    dev = torch.device("cuda", 0)
    env = pkg.envs.VecEnv(4, curriculum_config=cfg_of("easy"), reward_type="dense", max_episode_steps=40, device=dev)
    env.set_curricula([cfg_of("easy")])
    pol = E.policy_of(PARAMS, deterministic=False, seed=1)
    packed, params, std = pol.device_tensors(dev)
    p = evr.EpisodeProgram([cfg_of("easy")], "dense", max_episode_steps=40)
    p.add_lane([evr.Segment(0, [1], 0.05, 0.05, noise_seed=3)])
    plan = p.plan()
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    lane, seg = t(plan.lane_off, torch.int32), torch.from_numpy(plan.segments.view(np.uint8).copy()).to(dev)
    tapes = {"reset_tape": t(plan.reset, torch.float64), "noise_tape": t(plan.noise, torch.float64),
             "policy_tape": torch.zeros(1, 15 * 40, dtype=torch.float64, device=dev)}
    ret = torch.zeros(1, dtype=torch.float64, device=dev)
    length = torch.full((1,), -1, dtype=torch.int32, device=dev)
    suc = torch.zeros(1, dtype=torch.uint8, device=dev)
    queue, status = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def args(policy=N.EVAL_POLICY_MLP, period=0, tape=None):
        a = N.EvalArgs()
        a.num_lanes, a.policy, a.max_steps, a.total_episodes = 1, policy, 40, 1
        a.lane_segments, a.segments = N.ptr(lane), N.ptr(seg)
        a.ep_return, a.ep_length, a.ep_success = N.ptr(ret), N.ptr(length), N.ptr(suc)
        a.status, a.work_queue, a.stream_period = N.ptr(status), N.ptr(queue), period
        if tape is not None:
            setattr(a, tape, N.ptr(tapes[tape]))
            a.policy_stride = 15 * 40
        return a

    m = N.EvalMlp()
    m.packed, m.params, m.action_std = N.ptr(packed), N.ptr(params), N.ptr(std)
    call = lambda a: N.call("dxrl_evaluate_mlp", env.handle, C.byref(a), C.byref(m), N.stream_of(dev))  # noqa: E731
    with pytest.raises(ValueError, match="stream_period must be >= 0"):
        call(args(period=-1))
    for tape in tapes:
        with pytest.raises(ValueError, match="parity tape"):
            call(args(period=1, tape=tape))
    for policy in (N.EVAL_POLICY_SIMPLE, N.EVAL_POLICY_HEURISTIC, N.EVAL_POLICY_RANDOM):
        for period in (1, -1):
            with pytest.raises(ValueError, match="stream_period"):
                N.call("dxrl_evaluate", env.handle, C.byref(args(policy, period)), N.stream_of(dev))
    torch.cuda.synchronize()
    assert length.item() == -1 and status.item() == 0 and queue.item() == 0  # nothing ran
    call(args(period=1))  # the same arguments with a valid period: one episode
    torch.cuda.synchronize()
    assert 1 <= length.item() <= 40 and status.item() == 0
    env.close()
    # the Python surface
    prog = evr.policy_program(pol)
    kw = dict(host_resets=False, host_noise=False)
    with pytest.raises(ValueError, match="stream_period"):
        p.run(prog, stream_period=-1, **kw)
    with pytest.raises(ValueError, match="host_resets"):
        p.run(prog, stream_period=1, host_noise=False)
    with pytest.raises(ValueError, match="host_resets"):
        p.run(prog, stream_period=1, host_resets=False)
    with pytest.raises(ValueError, match="host_resets"):
        p.run(prog, stream_period=1, policy_tapes=np.zeros((1, 600)), **kw)

    class HeuristicPolicy:  # the reference's name: compiled as DXRL_EVAL_POLICY_HEURISTIC
        pass

    with pytest.raises(ValueError, match="MLP actor"):
        p.run(evr.policy_program(HeuristicPolicy()), stream_period=1, **kw)
