"""GPU: every env-step implementation on the crafted edge lanes of tests/env_edge_cases.py.

The env's formulas are stated once (csrc/dxrl_device.h: joint_step, object_axis_step,
dense_reward_of, sparse_reward, the flag-word transitions, the reset tail) but scheduled four ways
-- the scalar env_step, and the lane-split forms in dxrl_pg_rollout16.hip, dxrl_pg_rollout8.hip
and dxrl_eval_row.h, the last one compiled into both k_eval_ls and k_eval_mlp: which lanes compute,
which commit, in which phase and through which LDS records -- and run in five kernel families.  States
from ordinary resets and policies never take the x / y wall stops, the z ceiling, the joint clip,
sqrt_below()'s exact-root branch, most contact / previous-contact combinations or the truncation
bounds; these lanes do (tests/test_env_edge_cases_host.py proves it on the CPU, and every test
here runs the same checker first).  Everything is compared with the pinned CPU oracle bit for bit,
except rewards, which keep the project's bars (1e-12 relative in f64, one f32 ulp on the
policy-gradient tape)."""
import math

import numpy as np
import pytest
import torch

import env_edge_cases as E

pytestmark = pytest.mark.gpu

REW_RTOL = 1e-12  # test_gpu_parity.py's bar for f64 rewards (np.exp vs libm: <= 1 ulp)
T = E.T


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import envs, trainer, evaluator  # noqa: F401
    assert torch.cuda.is_available()
    return d


@pytest.fixture(scope="module")
def state_cases():
    cases = E.build("state")
    return cases, E.check(cases)


@pytest.fixture(scope="module")
def reset_cases():
    cases = E.build("reset")
    return cases, E.check(cases)


def bits(x):
    """The bit pattern of a float array (-0.0 and 0.0 differ)."""
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def write_slab(env, cases):
    """The lanes' states into the VecEnv's state slab."""
    dev = env.device
    put = lambda view, a: view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))  # noqa: E731
    put(env.joint_positions, cases.stack("jp", np.float32).T)
    put(env.joint_velocities, cases.stack("jv", np.float32).T)
    put(env.object_position, cases.stack("op", np.float64).T)
    put(env.object_velocity, cases.stack("ov", np.float32).T)
    put(env.flags, cases.flags().view(np.int32))
    put(env.step_count, cases.stack("t", np.int32))
    put(env.object_size, cases.stack("size", np.float64))
    put(env.object_mass, cases.stack("mass", np.float64))
    put(env.friction_coefficient, cases.stack("fric", np.float64))
    torch.cuda.synchronize(dev)


def read_slab(env):
    return dict(jp=env.joint_positions.cpu().numpy().T, jv=env.joint_velocities.cpu().numpy().T,
                op=env.object_position.cpu().numpy().T, ov=env.object_velocity.cpu().numpy().T,
                flags=env.flags.cpu().numpy().view(np.uint32), t=env.step_count.cpu().numpy())


def flags_after_step(ln, mask):
    """The flag word after a dense step that found contacts ``mask``."""
    return mask | (mask << E.PREV_SHIFT) | E.HAS_PREV | E.HAS_OBJECT | (E.FRIC_F64 if ln.fric_f64 else 0)


def assert_state(got, i, want, ln, name):
    """Slab state of lane i == the oracle's state ``want`` (a trace entry after a step)."""
    assert np.array_equal(bits(got["jp"][i]), bits(np.array(want["jp"], np.float32))), (name, "jp")
    assert np.array_equal(bits(got["jv"][i]), bits(np.array(want["jv"], np.float32))), (name, "jv")
    assert np.array_equal(bits(got["op"][i]), bits(np.array(want["op"], np.float64))), (name, "op")
    assert np.array_equal(bits(got["ov"][i]), bits(np.array(want["ov"], np.float32))), (name, "ov")
    assert got["flags"][i] == flags_after_step(ln, want["mask"]), (name, hex(got["flags"][i]))
    assert got["t"][i] == want["t"], (name, "t")


def step_and_compare(env, cases, traces):
    acts = torch.from_numpy(cases.actions()).to(env.device)
    for s in range(T):
        ob, rw, te, tr = (x.cpu().numpy() for x in env.step(acts[s].contiguous()))
        got = read_slab(env)
        for i, ln in enumerate(cases.lanes):
            w, name = traces[i][s], (ln.name, s)
            assert np.array_equal(bits(ob[i]), bits(w["obs"])), (name, np.flatnonzero(ob[i] != w["obs"]))
            assert math.isclose(rw[i], w["reward"], rel_tol=REW_RTOL, abs_tol=1e-15), (name, rw[i], w["reward"])
            assert (bool(te[i]), bool(tr[i])) == (w["term"], w["trunc"]), name
            assert_state(got, i, w, ln, name)


# ------------------------------------------------------------------ 1. dxrl_env_step / dxrl_env_reset
def test_env_step_on_edge_states(pkg, state_cases):
    """k_step (the scalar env_step) from slab states: observation, state and flags bit for bit,
    reward to 1e-12, on every lane and step -- the special-action lanes included."""
    cases, traces = state_cases
    env = pkg.envs.VecEnv(len(cases), reward_type="dense", max_episode_steps=cases.max_episode_steps)
    env.reset(write_obs=False)
    write_slab(env, cases)
    obs0 = env.observe().cpu().numpy()
    for i, ln in enumerate(cases.lanes):
        assert np.array_equal(bits(obs0[i]), bits(traces[i][-1]["obs"])), ln.name
    step_and_compare(env, cases, traces)
    env.close()


def test_env_reset_and_step_on_edge_draws(pkg, reset_cases):
    """k_reset from resolved draws (the reset-time knife edge: ME:176 contacts with the size a few
    ulps around d / 1.5; spawns beyond the walls), then k_step from those states."""
    cases, traces = reset_cases
    C = pkg.experiments.CurriculumConfig
    L = len(cases)
    env = pkg.envs.VecEnv(L, reward_type="dense", max_episode_steps=cases.max_episode_steps)
    env.set_curricula([C(**kw) for kw, _ in E.reset_curricula()], env_index=cases.rows())
    dev = env.device
    obs0 = env.reset(mask=torch.ones(L, dtype=torch.uint8, device=dev),
                     draws=torch.from_numpy(cases.reset_draws()).to(dev)).cpu().numpy()
    got = read_slab(env)
    size = env.object_size.cpu().numpy()
    for i, ln in enumerate(cases.lanes):
        w = traces[i][-1]
        assert np.array_equal(bits(obs0[i]), bits(w["obs"])), ln.name
        assert got["flags"][i] == (w["mask"] | E.OP_IS_F32 | E.HAS_OBJECT | (E.FRIC_F64 if ln.fric_f64 else 0)), ln.name
        assert size[i] == ln.size and got["t"][i] == 0, ln.name
        assert np.array_equal(bits(got["op"][i]), bits(np.array(w["op"]))), ln.name
    step_and_compare(env, cases, traces)
    env.close()


# ------------------------------------------------------------------ 2. the policy-gradient rollouts
PG_KERNELS = {16: "k_pg_rollout", 2048: "k_pg_rollout_ws", 1024: "k_pg_rollout_e8"}
_TAPES = ("obs_rm", "act", "logp", "rew", "done", "ep_ret", "ep_count", "rec_return", "rec_length", "rec_end")
_VIEWS = ("joint_positions", "joint_velocities", "object_position", "object_velocity", "flags", "step_count",
          "object_size", "friction_coefficient")


def _pg_rollout(pkg, cases, diag, saturate, max_steps, sizes=None):
    n = len(cases)
    env = pkg.envs.VecEnv(n, curriculum_config=pkg.CurriculumConfig.variable(), reward_type="dense", seed=11,
                          max_episode_steps=cases.max_episode_steps)
    cfg = pkg.trainer.TrainerConfig(horizon=T, seed=5, max_steps=max_steps, record_cap=T)
    tr = pkg.trainer.PGTrainer(env, cfg)
    env.reset(write_obs=False)
    write_slab(env, cases)
    if sizes is not None:
        env.object_size.copy_(torch.from_numpy(sizes).to(env.device))
    if saturate:  # sigma = e^3: most actions leave [-1, 1] and are clipped by the env step
        off = pkg.trainer.OFF["logstd"]
        tr.params[off:off + 15].fill_(3.0)
    tr.diag_flags = diag
    tr.rollout()
    torch.cuda.synchronize()
    out = {k: getattr(tr, k).clone() for k in _TAPES}
    out.update({k: getattr(env, k).clone() for k in _VIEWS})
    return env, tr, out


def _knife_sizes_for_policy(cases, act0):
    """The rollout draws its own actions, so the builder's post-step knife-edge sizes (made for the
    builder's action table) are off the edge there.  Step 0's action does not depend on the size
    (the observation does not show it), so a first rollout gives the action, the oracle the
    distance after step 0 under it, and the lane's size is d / 1.5 moved by the lane's k ulps."""
    sizes = cases.stack("size", np.float64)
    lanes = []
    for i, ln in enumerate(cases.lanes):
        if ln.family == "knife" and ln.cell[0] == "post0":
            o = E.oracle_of(cases, i)
            o.step(act0[i, :15])
            sizes[i] = E.ulps(o.dist[ln.cell[1]] / 1.5, ln.cell[2])
            lanes.append(i)
    return sizes, lanes


@pytest.mark.parametrize("saturate,max_steps", [(False, E.PG_MAX_STEPS), (True, E.MAX_EPISODE_STEPS + 50)],
                         ids=["policy", "saturated"])
def test_pg_rollout_kernels_on_edge_states(pkg, state_cases, saturate, max_steps):
    """k_pg_rollout (diag 16), k_pg_rollout_ws (2048) and k_pg_rollout_e8 (1024) from the edge
    states: the three equal bit for bit, and each lane replayed by the oracle on the action tape up
    to its first episode end gives the done flags exactly, the next observation rows after bf16
    rounding and the tape reward within one f32 ulp (test_gpu_fullsize.py's bar); lanes that never
    reset end in the oracle's state bit for bit (what sees a clip that bf16 hides).

    The tape shows only done = terminated | truncated | step count >= max_steps.  With max_steps
    (150) below the env's max_episode_steps (200) every truncation is also a rollout end, so the
    "policy" run pins the rollout's bound (lanes entering at 148 / 149 / 150) and the "saturated"
    run, with max_steps 250, the truncation bound (lanes entering at 198 / 199 / 200)."""
    cases, _ = state_cases
    n = len(cases)
    # pass 1 (the one-lane kernel): step 0's actions, for the knife-edge sizes under this policy
    _, tr0, _ = _pg_rollout(pkg, cases, 16, saturate, max_steps)
    sizes, knife = _knife_sizes_for_policy(cases, tr0.act.view(T, n, 16)[0].cpu().numpy())
    assert len(knife) == 25
    outs = {}
    for diag in PG_KERNELS:
        env, tr, outs[diag] = _pg_rollout(pkg, cases, diag, saturate, max_steps, sizes)
    for diag in (2048, 1024):
        for key, a in outs[16].items():
            assert torch.equal(a, outs[diag][key]), (PG_KERNELS[diag], key)
    o = {k: v.cpu().numpy() for k, v in outs[2048].items() if k != "obs_rm"}
    obs = outs[2048]["obs_rm"].view(T + 1, n, 64).float().cpu().numpy()
    act, rew, done = o["act"].reshape(T, n, 16), o["rew"].reshape(T, n), o["done"].reshape(T, n)
    end = dict(jp=o["joint_positions"].T, jv=o["joint_velocities"].T, op=o["object_position"].T,
               ov=o["object_velocity"].T, flags=o["flags"].view(np.uint32), t=o["step_count"])
    survivors = in_band = clipped = 0
    relations = set()
    for i, ln in enumerate(cases.lanes):
        orc = E.oracle_of(cases, i)
        orc.size = float(sizes[i])
        orc._contacts()
        ob = orc.obs()
        ob[40:45] = [(ln.contacts >> f) & 1 for f in range(5)]  # row 0 shows the slab's contact bits
        assert np.array_equal(obs[0, i, :45], bf16(ob)), ln.name
        ended = False
        for t in range(T):
            a = act[t, i, :15]
            clipped += int(np.sum(np.abs(a) > 1.0))
            ob, r, te, trn = orc.step(a)
            if i in knife and t == 0:
                f = ln.cell[1]
                s = E.snap(orc)
                in_band += E.in_band(s, f)
                relations.add(np.sign(s["dist"][f] - s["thr"]))
            r32 = np.float32(r)
            assert abs(rew[t, i] - r32) <= np.spacing(abs(r32)), (ln.name, t, rew[t, i], r)
            d = te or trn or orc.t >= max_steps
            assert bool(done[t, i]) == d, (ln.name, t)
            if d:
                ended = True
                break
            assert np.array_equal(obs[t + 1, i, :45], bf16(ob)), (ln.name, t)
        if not ended:
            survivors += 1
            assert_state(end, i, E.snap(orc), ln, ln.name)
    assert in_band == len(knife) and len(relations) >= 2, (in_band, relations)
    assert survivors > n // 3
    if saturate:
        assert clipped > 0.8 * 15 * survivors * T, clipped


# ------------------------------------------------------------------ 3. the evaluation kernels
def _eval_program(pkg, cases, max_episode_steps):
    evr = pkg.evaluator
    draws = cases.reset_draws()

    class TapeProgram(evr.EpisodeProgram):
        def _reset_tape(self, segs):
            return draws.copy(), draws[:, 15:18].copy()

    C = pkg.experiments.CurriculumConfig
    p = TapeProgram([C(**kw) for kw, _ in E.reset_curricula()], "dense", max_episode_steps=max_episode_steps,
                    max_steps=T)
    for row in cases.rows():
        p.add_lane([evr.Segment(int(row), [0])])
    return p


def _replay(cases, i, actions, max_episode_steps):
    """OracleEnv of lane i on the device's actions: (observations, return, length, success,
    contact history)."""
    o = E.oracle_of(cases, i, max_episode_steps=max_episode_steps)
    obs, hist, total, te = [o.obs()], [], 0.0, False
    for s in range(T):
        ob, r, te, tr = o.step(actions[s])
        obs.append(ob)
        total += r
        hist.append(o.num_contacts)
        if te or tr:
            break
    return np.stack(obs), total, len(hist), te, hist


def _assert_eval(cases, rec, mes, exact_actions):
    ends = 0
    for i, ln in enumerate(cases.lanes):
        n = int(rec.ep_length[i])
        if exact_actions is not None:  # the policy is the tape: the device's actions are the table's, clipped
            want = np.clip(exact_actions[:n, i], np.float32(-1), np.float32(1))
            assert np.array_equal(rec.act_traj[i, :n], want), ln.name
        obs, total, length, te, hist = _replay(cases, i, rec.act_traj[i], mes)
        assert n == length, (ln.name, n, length)
        assert np.array_equal(bits(rec.obs_traj[i, :n + 1]), bits(obs)), (ln.name, mes)
        assert bool(rec.ep_success[i]) == te and rec.ep_contacts[i] == hist[-1], ln.name
        assert rec.contact_hist[i, :n].tolist() == hist and not rec.contact_hist[i, n:].any(), ln.name
        assert math.isclose(rec.ep_return[i], total, rel_tol=1e-12, abs_tol=1e-15), (ln.name, rec.ep_return[i], total)
        ends += n < T
    return ends


@pytest.mark.parametrize("mes", [200, 2, 1, 0], ids=lambda m: f"max_episode_steps={m}")
def test_eval_ls_on_edge_resets(pkg, reset_cases, mes, monkeypatch):
    """k_eval_ls from a reset tape holding the edge lanes, the policy tape holding the lanes' action
    table (SimpleLearner program, mean 0, sigma 1: the action is the draw): trajectories, lengths,
    success, contacts and histories bit for bit against OracleEnv, returns to 1e-12; the one-lane
    k_eval gives equal records.  max_episode_steps 2 / 1 / 0 put the truncation bound (step count
    >= bound before the increment) at step 2 / 1 / 0 of every lane."""
    cases, _ = reset_cases
    evr, N = pkg.evaluator, pkg._native
    p = _eval_program(pkg, cases, mes)
    prog = evr._PolicyProgram(N.EVAL_POLICY_SIMPLE, np.zeros(15, np.float32), 1.0, None, None)
    acts = cases.actions()                                             # [T][L][15]
    tapes = np.ascontiguousarray(acts.transpose(1, 0, 2).reshape(len(cases), T * 15).astype(np.float64))
    recs = []
    for one in ("0", "1"):
        monkeypatch.setenv("DXRL_EVAL_ONE_LANE", one)
        recs.append(p.run(prog, policy_tapes=tapes, trajectories=True))
    rec, one = recs
    ends = _assert_eval(cases, rec, mes, acts)
    if mes < T:
        assert np.all(rec.ep_length <= mes + 1)
        assert np.sum(rec.ep_length == mes + 1) > len(cases) // 2
    else:
        assert ends >= 16  # the mask-grid lanes with >= 3 contacts terminate
    for k in ("ep_return", "ep_length", "ep_success", "ep_contacts", "contact_hist", "policy_used"):
        assert np.array_equal(getattr(rec, k), getattr(one, k)), k
    for i, n in enumerate(rec.ep_length.astype(int)):
        assert np.array_equal(bits(rec.obs_traj[i, :n + 1]), bits(one.obs_traj[i, :n + 1])), i
        assert np.array_equal(bits(rec.act_traj[i, :n]), bits(one.act_traj[i, :n])), i


@pytest.mark.parametrize("mode,mes", [("table", 200), ("table", 1), ("saturated", 200)])
def test_eval_mlp_on_edge_resets(pkg, reset_cases, mode, mes):
    """k_eval_mlp from the same reset tape.  "table": an actor whose head is zero (mu = 0) with
    std 1, so the action is the policy tape's draw -- the lanes' action table, and every named edge
    is met exactly; "saturated": a random actor with draws of +-50, so nearly every action is
    clipped.  Compared with OracleEnv on the device's actions as test_eval_ls_on_edge_resets does."""
    import eval_mlp_reference as M
    import pg_reference as R
    cases, _ = reset_cases
    evr = pkg.evaluator
    params = M.actor_params(3, logstd=0.0)
    acts = cases.actions()
    if mode == "table":
        R.unpack(params)["W3a"].zero_()
        draws = acts.transpose(1, 0, 2).astype(np.float64)
    else:
        rng = np.random.default_rng(17)
        draws = np.where(rng.random((len(cases), T, 15)) < 0.5, -50.0, 50.0)
    pol = M.policy_of(params, deterministic=False, seed=1)
    assert mode != "table" or not pol.W3a.any()
    p = _eval_program(pkg, cases, mes)
    rec = p.run(evr.policy_program(pol), policy_tapes=np.ascontiguousarray(draws.reshape(len(cases), T * 15)),
                trajectories=True)
    ends = _assert_eval(cases, rec, mes, acts if mode == "table" else None)
    if mode == "saturated":
        live = np.concatenate([rec.act_traj[i, :int(n)].ravel() for i, n in enumerate(rec.ep_length)])
        assert np.mean(np.abs(live) == 1.0) > 0.95
    assert ends >= 16
