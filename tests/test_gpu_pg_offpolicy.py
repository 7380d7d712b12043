"""GPU: the policy-gradient learner against the independent references (tests/pg_reference.py: the
bf16-emulating torch restatement and the same objective in fp64) in the states the rest of the suite
leaves out: ratios away from 1 on both sides of both clip boundaries (old log-probabilities
perturbed by pg_reference.offpolicy_logp, so the branch `s1 <= s2 || ratio == rc` is decided both
ways for both advantage signs), weights away from the initial ones (pg_reference.trained_like_params:
nonzero biases, actor head gain 0.5, 15 distinct log_std), minibatch slices that start inside a
tile, non-default loss coefficients -- and the loss statistics (policy_loss, value_mse, clip_frac,
approx_kl) against the references' per-sample terms.

Conditions on the inputs (asserted on the references, never on the kernel) in every off-policy
case: both references keep every sample's log ratio >= 0.04 from both clip boundaries, so the
clipped set is the same for any log pi within 0.04 of theirs and no sample has to be excluded; the
four advantage-sign x clipped-side combinations hold >= 5 % of the rows each.

The 10 x condition on policy_loss and approx_kl (their fp64 value against the statistic's tolerance)
is asserted in the off-policy cases; on-policy both values are 0 by construction (ratio exactly 1,
normalised advantages) and the kernel's own approx_kl must be 0 instead.

First MI355X run, all cases (DESIGN.md section 5 has each): pin ratios |hip - fp64| /
|bf16 torch - fp64| 0.96 .. 1.02 for every gradient block, bias column, logstd, V, adv, log pi and
mu (b3c, one scalar: 0.51 .. 1.00) against the bound 1.5; margins 0.070 .. 0.088; rarest sign x side
combination 5.6 % (5 x 32) .. 8.9 %; clip counts equal; |policy_loss - fp64| <= 5.7e-4 (tolerance
3.3e-3 .. 4.0e-3, trained-like), |approx_kl - fp64| <= 3.4e-4 (tolerance 5.0e-3), |value_mse -
fp64| <= 4.7e-3 (tolerance 4.3e-3 .. 1.3e-2)."""
import pytest
import torch

import pg_reference as R

pytestmark = pytest.mark.gpu

FACTOR = 1.5  # the project's own bound (pg_reference.fp64_pin)
# Bounds other than 1.5, by quantity, each with its cause (none measured above 1.5 so far).
PIN_FACTORS = {}
MARGIN = 0.04
QUADRANT = 0.05


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import envs, trainer  # noqa: F401
    return d


def make(pkg, n, T, ent_coef=0.01, **kw):
    """As test_gpu_pg.make: variable curriculum, dense reward."""
    env = pkg.envs.VecEnv(n, curriculum_config=pkg.CurriculumConfig.variable(), reward_type="dense", seed=3)
    cfg = pkg.trainer.TrainerConfig(horizon=T, seed=1, ent_coef=ent_coef, **kw)
    tr = pkg.trainer.PGTrainer(env, cfg)
    env.reset(write_obs=False)
    return env, tr


def collect(tr, trained, eps_seed):
    """Rollout, values and advantages (under trained-like weights if asked); then, if eps_seed is not
    None, the old log-probabilities moved off-policy.  Only tr.logp changes after the rollout, so the
    stored layer-2 tapes stay valid.  Returns the rollout's own log pi."""
    if trained:
        tr.params.copy_(R.trained_like_params(5).to(tr.dev))
        tr.pack()
    tr.rollout()
    (tr.critic_values if tr.cfg.fused else tr.critic_forward)()
    tr.advantages()
    logp_roll = tr.logp.clone()
    if eps_seed is not None:
        tr.logp.copy_(R.offpolicy_logp(tr.logp, tr.cfg.clip_eps, eps_seed))
    return logp_roll


def train(tr, rows=None):
    """The train passes of one step without the optimiser step, on whichever learner path tr has."""
    if tr.cfg.fused:
        if rows is not None:
            tr._mb = rows
        tr.train_passes()
    else:
        assert rows is None
        tr.actor_forward()
        tr.heads()
        tr.backward()
    torch.cuda.synchronize()


def cfg_of(tr):
    c = tr.cfg
    return dict(gamma=c.gamma, lam=c.lam, clip_eps=c.clip_eps, vf_coef=c.vf_coef, ent_coef=c.ent_coef)


def check(tr, n, T, logp_roll, offpolicy, rows=None, label=""):
    """Every check of the module on a finished train pass; prints each figure before asserting."""
    cfg = cfg_of(tr)
    eps = cfg["clip_eps"]
    M = n * T
    start, count = rows or (0, M)
    sl = slice(start, start + count)
    tape = (tr.obs_rm, tr.act, tr.logp, tr.rew, tr.done, n, T, cfg)
    g_b, info_b = R.loss_and_grads(tr.params.clone(), *tape, bf16=True, rows=rows)
    g_64, info_64 = R.loss_and_grads(tr.params.double(), *tape, bf16=False, rows=rows)
    tb, t64 = info_b["terms"], info_64["terms"]

    # ---- conditions on the inputs (the references alone)
    margins = (R.ratio_margin(info_b, eps), R.ratio_margin(info_64, eps))
    quads = (R.clip_quadrants(info_b, eps), R.clip_quadrants(info_64, eps))
    print(f"\n[{label}] rows {count} margin bf16 {margins[0]:.4f} fp64 {margins[1]:.4f} quadrants "
          + " ".join(f"{k} {v:.3f}" for k, v in quads[1].items()))
    if offpolicy:
        assert min(margins) >= MARGIN, margins
        assert torch.equal(tb["clip"], t64["clip"])  # no sample excluded: both references clip the same set
        for q in quads:
            assert all(v >= QUADRANT for v in q.values()), q
    else:  # on-policy: the references' ratios stay inside the clip range, as far from its boundaries
        assert min(margins) >= MARGIN and not tb["clip"].any() and not t64["clip"].any(), margins

    # ---- fp64 pin: gradient blocks, bias columns, logstd, V, adv, the rollout's log pi (and mu)
    extra = {}
    if not tr.cfg.fused:  # the fused kernel never materialises mu
        extra["mu"] = (tr.mu[:, :15], info_b["mu"][:, :15], info_64["mu"][:, :15])
    pin = lambda **kw: R.fp64_pin(tr.grads, tr.V[0], tr.adv, tr.params.clone(), *tape, g_b, info_b,  # noqa: E731
                                  blocks=R.ALL_BLOCKS, rows=rows, truth=(g_64, info_64),
                                  logp=(logp_roll[sl], info_b["lp"], info_64["lp"]), extra=extra, **kw)
    ratios = pin(factor=float("inf"))
    print(f"[{label}] pin " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    print(f"[{label}] |logp - fp64| max: rollout {(logp_roll[sl].double() - info_64['lp']).abs().max().item():.4f} "
          f"bf16 torch {(info_b['lp'].double() - info_64['lp']).abs().max().item():.4f}")

    # ---- loss statistics
    s = tr.loss_stats()
    got_clip = s["clip_frac"] * count
    want_clip = int(t64["clip"].sum().item())
    stat = {}
    for name, key in (("policy_loss", "policy"), ("value_mse", "value"), ("approx_kl", "kl")):
        ref = t64[key].mean().item()
        tol = 2.0 * (tb[key].double() - t64[key]).abs().mean().item()
        stat[name] = (s[name], ref, tol)
    print(f"[{label}] clip count {got_clip:.6f} want {want_clip} | "
          + " | ".join(f"{k} got {g:.6g} fp64 {r:.6g} tol {t:.3g}" for k, (g, r, t) in stat.items()))

    pin(factor=FACTOR, factors=PIN_FACTORS)
    assert want_clip < 2 ** 24 and abs(got_clip - want_clip) < 1e-6, (got_clip, want_clip)
    if offpolicy:
        assert want_clip == int(tb["clip"].sum().item()) and 0.4 * count < want_clip < 0.6 * count
    for name, (got, ref, tol) in stat.items():
        assert abs(got - ref) <= tol, (name, got, ref, tol)
        if offpolicy and name != "value_mse":  # a sign or branch error cannot hide inside the tolerance
            assert abs(ref) >= 10.0 * tol, (name, ref, tol)
    if not offpolicy and tr.cfg.fused:  # rollout log pi == training log pi bit for bit: ratio exactly 1
        assert s["clip_frac"] == 0.0 and abs(s["approx_kl"]) < 1e-9
    return ratios


PATHS = {"paired": {}, "per_network": dict(pair_learner=False), "gemm_chain": dict(fused=False)}


@pytest.mark.parametrize("path", list(PATHS))
def test_offpolicy_trained_like_matches_references(pkg, path):
    """256 x 32, trained-like weights, ratios on both sides of both clip boundaries, through all
    three head implementations: k_pg_fused's paired step, its per-network passes, k_ppo_heads."""
    n, T = 256, 32
    _, tr = make(pkg, n, T, **PATHS[path])
    assert tr.paired == (path == "paired")
    logp_roll = collect(tr, True, 21)
    train(tr)
    check(tr, n, T, logp_roll, True, label=f"trained offpolicy {path}")


@pytest.mark.parametrize("n", [773, 5])
def test_offpolicy_ragged_tiles(pkg, n):
    """773 x 32: a ragged last 128-sample tile; 5 x 32: one partial tile (per-network passes: too
    few dW2 chunks for the paired step)."""
    T = 32
    _, tr = make(pkg, n, T)
    assert tr.paired == (n == 773)
    logp_roll = collect(tr, True, 22)
    train(tr)
    check(tr, n, T, logp_roll, True, label=f"trained offpolicy {n}x{T}")


def test_offpolicy_minibatch_slice_inside_a_tile(pkg):
    """772 x 32 as a 4-minibatch PPO trainer runs it: the pass over samples q .. 3q - 1 (q = M / 4 =
    48 tiles + 32 samples) starts inside a 128-sample tile; logp, act, adv, ret and the stored
    actor H2 are read at that offset, the advantage moments stay the whole tape's
    (pg_reference rows=)."""
    n, T = 772, 32
    _, tr = make(pkg, n, T, minibatches=4)
    q = tr.M // 4
    assert tr.paired and q % 32 == 0 and q % 128 and tr.minibatch_bounds()[1] == q
    logp_roll = collect(tr, True, 23)
    train(tr, rows=(q, 2 * q))
    check(tr, n, T, logp_roll, True, rows=(q, 2 * q), label="trained offpolicy 772x32 slice (q, 2q)")


def test_offpolicy_non_default_coefficients(pkg):
    n, T = 256, 32
    _, tr = make(pkg, n, T, clip_eps=0.1, vf_coef=1.0, ent_coef=0.02, gamma=0.9, lam=0.8)
    logp_roll = collect(tr, True, 24)
    train(tr)
    check(tr, n, T, logp_roll, True, label="trained offpolicy eps 0.1 vf 1.0 ent 0.02 gamma 0.9 lam 0.8")


def test_offpolicy_initial_weights(pkg):
    """The ratio logic alone: initial weights (mu ~ 0, zero biases), off-policy log-probabilities."""
    n, T = 256, 32
    _, tr = make(pkg, n, T)
    logp_roll = collect(tr, False, 25)
    train(tr)
    check(tr, n, T, logp_roll, True, label="initial offpolicy")


@pytest.mark.parametrize("path", ["paired", "gemm_chain"])
def test_onpolicy_trained_like_matches_references(pkg, path):
    """The weight state alone: trained-like weights, the rollout's own log-probabilities."""
    n, T = 256, 32
    _, tr = make(pkg, n, T, **PATHS[path])
    logp_roll = collect(tr, True, None)
    train(tr)
    check(tr, n, T, logp_roll, False, label=f"trained onpolicy {path}")


def test_offpolicy_paired_equals_per_network_bit_for_bit(pkg):
    """test_paired_learner_equals_two_passes at ratio != 1 and trained-like weights: the paired step
    and two per-network calls at the same dW2 split count give the same gradients and loss sums
    bit for bit, full batch and a slice that starts inside a tile."""
    n, T = 772, 32
    outs = []
    for paired in (True, False):
        _, tr = make(pkg, n, T, minibatches=4)
        assert tr.paired
        if not paired:
            tr.paired = False
            tr.splits = tr.pair_splits
            tr.kpartial = torch.zeros(tr.splits + 16, 256, 288, device=tr.dev)
        collect(tr, True, 23)
        q = tr.M // 4
        got = []
        for rows in ((q, 2 * q), (0, tr.M)):
            train(tr, rows=rows)
            got.append((tr.grads.clone(), tr.fused_loss.clone()))
        outs.append(got)
    for (ga, la), (gb, lb) in zip(*outs):
        assert torch.equal(ga, gb) and torch.equal(la, lb)
        assert la[:, 2].sum() > 0  # clipped samples on this tape
