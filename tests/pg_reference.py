"""Plain-PyTorch fp32 reference of the policy-gradient learner (test-only).

The reference repository has no network / GAE / policy gradient, so this
restatement pins the HIP learner instead ("parity unpinned vs the
reference").  `loss_and_grads(..., bf16=True)` rounds to bf16 at exactly the
points the HIP pipeline stores bf16 (obs, weights, hidden activations,
head gradients, hidden gradients); `bf16=False` is the exact fp32 math,
checked against autograd in the CPU tests.
"""
import math

import torch

OBS_IN, IN, H, HX, OUT, ACT = 45, 64, 256, 288, 32, 15
W1, W2, W3 = H * IN, H * HX, OUT * HX
OFF = {"W1a": 0, "W2a": W1, "W3a": W1 + W2, "logstd": W1 + W2 + W3}
OFF["W1c"] = OFF["logstd"] + 32
OFF["W2c"] = OFF["W1c"] + W1
OFF["W3c"] = OFF["W2c"] + W2
NPARAMS = OFF["W3c"] + W3
LOG2PI = math.log(2 * math.pi)


def unpack(params):
    p = params
    blk = lambda name, r, c: p[OFF[name]:OFF[name] + r * c].view(r, c)  # noqa: E731
    out = {}
    for net in "ac":
        out[f"W1{net}"] = blk(f"W1{net}", H, IN)
        out[f"W2{net}"] = blk(f"W2{net}", H, HX)
        out[f"W3{net}"] = blk(f"W3{net}", OUT, HX)
    out["logstd"] = p[OFF["logstd"]:OFF["logstd"] + ACT]
    return out


def _r(x, bf16):
    return x.to(torch.bfloat16).float() if bf16 else x


def mlp_forward(X, Wd, net, bf16):
    """X [R][64] (col 45 = 1). Returns H1, H2 (stored precision) and the f32 head [R][32]."""
    W1_, W2_, W3_ = (_r(Wd[f"W{k}{net}"], bf16) for k in (1, 2, 3))
    b2 = Wd[f"W2{net}"][:, H]  # biases from the f32 master
    b3 = Wd[f"W3{net}"][:, H]
    H1 = _r(torch.tanh(X @ W1_.T), bf16)
    H2 = _r(torch.tanh(H1 @ W2_[:, :H].T + b2), bf16)
    head = H2 @ W3_[:, :H].T + b3
    return H1, H2, head


def gae_uses_segmented_scan(T):
    """dxrl_pg_gae's kernel choice (csrc/dxrl_pg_gae.hip): k_gae_lds (segmented scan) while the horizon's
    LDS staging fits 152 KiB, else k_gae (one sequential chain per env)."""
    pitch = (T + 7) // 8 * 8 + 4
    return 16 * (12 * pitch + 4 * T) <= 152 * 1024


def gae(rew, done, V, n, T, gamma, lam, scan=None):
    """rew/done [T*n], V [(T+1)*n] -> adv, ret [T*n] (f32, the kernel's formula order).
    scan (default: the kernel's choice for T): k_gae_lds's segmented wavefront scan -- the horizon
    padded to 8-step chunks, 16 segments of whole chunks per env composed into affine maps, a
    Hillis-Steele suffix scan over the segments, each segment rerun from its incoming value --
    restated op for op; else the one-chain sequential recurrence of k_gae."""
    if scan is None:
        scan = gae_uses_segmented_scan(T)
    if scan:
        return _gae_segmented(rew, done, V, n, T, gamma, lam)
    rew, done, V = rew.view(T, n), done.view(T, n).float(), V.view(T + 1, n)
    adv = torch.empty(T, n, dtype=rew.dtype, device=rew.device)
    next_adv = torch.zeros(n, dtype=rew.dtype, device=rew.device)
    next_v = V[T]
    g = torch.tensor(gamma, dtype=rew.dtype)
    lm = torch.tensor(lam, dtype=rew.dtype)
    for t in range(T - 1, -1, -1):
        nd = 1.0 - done[t]
        delta = rew[t] + g * next_v * nd - V[t]
        a = delta + g * lm * nd * next_adv
        adv[t] = a
        next_adv = a
        next_v = V[t]
    ret = adv + V[:T]
    return adv.reshape(-1), ret.reshape(-1)


def _gae_segmented(rew, done, V, n, T, gamma, lam):
    rew, done, V = rew.view(T, n), done.view(T, n).float(), V.view(T + 1, n)
    dt, dev = rew.dtype, rew.device
    g = torch.tensor(gamma, dtype=dt)
    gl = g * torch.tensor(lam, dtype=dt)
    T8 = (T + 7) // 8 * 8
    delta = torch.zeros(T8, n, dtype=dt, device=dev)
    c = torch.zeros(T8, n, dtype=dt, device=dev)
    delta[:T] = rew + g * V[1:] * (1.0 - done) - V[:T]
    c[:T] = torch.where(done > 0, torch.zeros((), dtype=dt, device=dev), gl.to(dev))
    nc, S = T8 // 8, 16
    seg = [(8 * (s * nc // S), 8 * ((s + 1) * nc // S)) for s in range(S)]
    D = [torch.zeros(n, dtype=dt, device=dev) for _ in range(S)]
    C = [torch.ones(n, dtype=dt, device=dev) for _ in range(S)]
    for s, (lo, hi) in enumerate(seg):  # each segment's affine map from A_in = 0
        for t in range(hi - 1, lo - 1, -1):
            D[s] = delta[t] + c[t] * D[s]
            C[s] = c[t] * C[s]
    off = 1
    while off < S:  # suffix scan, every lane reading its neighbour's value of the previous step
        D, C = ([D[s] + C[s] * D[s + off] if s + off < S else D[s] for s in range(S)],
                [C[s] * C[s + off] if s + off < S else C[s] for s in range(S)])
        off *= 2
    adv = torch.empty(T8, n, dtype=dt, device=dev)
    for s, (lo, hi) in enumerate(seg):
        a = D[s + 1] if s + 1 < S else torch.zeros(n, dtype=dt, device=dev)
        for t in range(hi - 1, lo - 1, -1):
            a = delta[t] + c[t] * a
            adv[t] = a
    adv = adv[:T]
    ret = adv + V[:T]
    return adv.reshape(-1), ret.reshape(-1)


def loss_and_grads(params, obs_rm, act, logp_old, rew, done, n, T, cfg, bf16=True, norm_stats=None, total=None,
                   world=1, scales=None, rows=None):
    """Manual forward/backward of the PPO objective as the HIP pipeline computes it.
    rows = (start, count): one minibatch pass as PGTrainer runs it -- V, GAE and the advantage
    moments over the whole tape, the gradient, the loss and info["terms"] over the samples
    start .. start + count - 1 alone, scaled by 1 / count (info["V"/"adv"/"ret"] stay whole).
    Sharded use (as PGTrainer with world > 1): norm_stats(adv) -> (mean, std) computed
    across ranks, total = global sample count, world = number of ranks; or
    scales = (per-sample loss scale, per-rank entropy coefficient) as
    distributed.loss_scales returns them (what the trainer hands the kernels).
    Returns (grads [NPARAMS], info dict)."""
    M = n * T
    start, count = (0, M) if rows is None else rows
    sl = slice(start, start + count)
    total = count if total is None else total
    inv_total, ent = (1.0 / total, cfg["ent_coef"] / world) if scales is None else scales
    Wd = unpack(params)
    dt = params.dtype
    X = obs_rm.to(dt)
    H1c, H2c, vhead = mlp_forward(X, Wd, "c", bf16)
    V_all = vhead[:, 0]
    adv_all, ret_all = gae(rew.to(dt), done, V_all, n, T, cfg["gamma"], cfg["lam"])
    if norm_stats is None:
        mean, std = adv_all.double().mean(), adv_all.double().std()
    else:
        mean, std = norm_stats(adv_all)
    A = ((adv_all.double() - mean) / (std + 1e-8)).to(dt)[sl]
    V, ret = V_all[sl], ret_all[sl]
    Xa = X[sl]
    H1a, H2a, muh = mlp_forward(Xa, Wd, "a", bf16)
    mu = muh[:, :ACT]
    ls = Wd["logstd"]
    a = act[sl, :ACT]
    logp_old = logp_old[sl]
    iv = torch.exp(-2.0 * ls)
    z = (a - mu) * torch.exp(-ls)
    lp = (-0.5 * z * z - ls - 0.5 * LOG2PI).sum(1)
    ratio = torch.exp(lp - logp_old)
    s1, s2 = ratio * A, torch.clamp(ratio, 1 - cfg["clip_eps"], 1 + cfg["clip_eps"]) * A
    rc = torch.clamp(ratio, 1 - cfg["clip_eps"], 1 + cfg["clip_eps"])
    gsel = torch.where((s1 <= s2) | (ratio == rc), -A * ratio, torch.zeros_like(A)) * inv_total
    d = a - mu
    dmu = gsel[:, None] * d * iv
    dls = (gsel[:, None] * (d * d * iv - 1.0)).sum(0) - ent
    dv = 2.0 * cfg["vf_coef"] * (V - ret) * inv_total
    grads = torch.zeros(NPARAMS, dtype=dt, device=params.device)
    G = unpack(grads)
    G["logstd"].copy_(dls)
    for net, dY, H1, H2 in (("a", dmu, H1a, H2a), ("c", dv[:, None], H1c[sl], H2c[sl])):
        k = dY.shape[1]
        dYr = _r(dY, bf16)
        W2_, W3_ = _r(Wd[f"W2{net}"], bf16), _r(Wd[f"W3{net}"], bf16)
        G[f"W3{net}"][:k, :H] = dYr.T @ H2
        G[f"W3{net}"][:k, H] = dYr.sum(0)
        dH2 = _r((dYr @ W3_[:k, :H]) * (1 - H2 * H2), bf16)
        G[f"W2{net}"][:, :H] = dH2.T @ H1
        G[f"W2{net}"][:, H] = dH2.sum(0)
        dH1 = _r((dH2 @ W2_[:, :H]) * (1 - H1 * H1), bf16)
        G[f"W1{net}"][:, :] = dH1.T @ Xa
    # per-sample loss terms (what the kernels sum into policy_loss, value_mse, clip_frac, approx_kl)
    terms = {"policy": -torch.minimum(s1, s2), "value": (V - ret) ** 2,
             "clip": (ratio - 1).abs() > cfg["clip_eps"], "kl": logp_old - lp}
    loss = terms["policy"].mean() + cfg["vf_coef"] * terms["value"].mean() - cfg["ent_coef"] * (
        ls.sum() + 0.5 * ACT * (1 + LOG2PI))
    return grads, {"V": V_all, "adv": adv_all, "ret": ret_all, "mu": muh, "mean": mean, "std": std, "loss": loss,
                   "ratio": ratio, "lp": lp, "logp_old": logp_old, "A": A, "terms": terms}


def autograd_loss(params, obs_rm, act, logp_old, rew, done, n, T, cfg, rows=None):
    """The same objective through torch autograd (fp64 OK); adv/ret/normalisation are constants.
    rows = (start, count): the mean loss over that slice of samples (moments over the whole tape)."""
    M = n * T
    start, count = (0, M) if rows is None else rows
    sl = slice(start, start + count)
    params = params.detach().clone().requires_grad_(True)
    Wd = unpack(params)
    X = obs_rm.to(params.dtype)
    with torch.no_grad():
        _, _, vh = mlp_forward(X, {k: v.detach() for k, v in Wd.items()}, "c", False)
        adv, ret = gae(rew.to(params.dtype), done, vh[:, 0], n, T, cfg["gamma"], cfg["lam"])
        A = ((adv - adv.mean()) / (adv.std() + 1e-8))[sl]
        ret = ret[sl]
    _, _, vh = mlp_forward(X[sl], Wd, "c", False)
    V = vh[:, 0]
    _, _, muh = mlp_forward(X[sl], Wd, "a", False)
    mu, ls = muh[:, :ACT], Wd["logstd"]
    a = act[sl, :ACT].to(params.dtype)
    lp = (-0.5 * ((a - mu) * torch.exp(-ls)) ** 2 - ls - 0.5 * LOG2PI).sum(1)
    ratio = torch.exp(lp - logp_old[sl].to(params.dtype))
    s1 = ratio * A
    s2 = torch.clamp(ratio, 1 - cfg["clip_eps"], 1 + cfg["clip_eps"]) * A
    loss = (-torch.minimum(s1, s2)).mean() + cfg["vf_coef"] * ((V - ret) ** 2).mean() - cfg["ent_coef"] * (
        ls.sum() + 0.5 * ACT * (1 + LOG2PI))
    loss.backward()
    return params.grad.detach()


BIAS_BLOCKS = {f"b{k}{net}": (f"W{k}{net}", OBS_IN if k == 1 else H) for k in (1, 2, 3) for net in "ac"}
GRAD_BLOCKS = ("W1a", "W2a", "W3a", "W1c", "W2c", "W3c")
ALL_BLOCKS = GRAD_BLOCKS + tuple(BIAS_BLOCKS) + ("logstd",)


def pin_block(grads, name):
    """A named piece of a [NPARAMS] vector: a weight block (its bias column included), a bias column
    on its own (b1a .. b3c: column 45 of W1, column 256 of W2 / W3) or logstd."""
    Wd = unpack(grads)
    if name in BIAS_BLOCKS:
        blk, col = BIAS_BLOCKS[name]
        return Wd[blk][:, col]
    return Wd[name]


def fp64_pin(got_grads, got_V, got_adv, params, obs_rm, act, logp_old, rew, done, n, T, cfg, g_bf16, info_bf16,
             factor=1.5, blocks=GRAD_BLOCKS, rows=None, logp=None, truth=None, factors=None, extra=None):
    """Pin the HIP learner to fp64 truth, not just to the bf16 restatement:
    the same objective on the same tapes in float64 with no bf16 rounding anywhere is the truth;
    for every gradient block and for V / adv the HIP result's distance to it must be at most
    `factor` x the bf16-emulating torch reference's distance (both carry the same bf16 storage
    points, so a kernel regression that adds error shows as a ratio above 1).  Returns the
    ratios {name: |hip - truth| / |bf16 ref - truth|}.
    blocks may also name the bias columns on their own (b1a, b2a, b3a, b1c, b2c, b3c: one column of
    257 barely moves its block's norm) and logstd; rows = (start, count) is the minibatch slice of
    loss_and_grads; logp = (got, ref, truth) pins log pi the same way, extra = {name: (got, ref,
    truth)} any further quantity (the GEMM chain's mu); truth = (grads, info) of the fp64 run when
    the caller already has it; factors = {name: factor} overrides `factor` for the
    named quantities (each with its cause written down where it is raised).  Every ratio is
    computed before the first assertion, so a failure reports all of them."""
    if truth is None:
        truth = loss_and_grads(params.double(), obs_rm, act, logp_old, rew, done, n, T, cfg, bf16=False, rows=rows)
    g64, info64 = truth
    ratios, bad = {}, []
    pairs = [(b, pin_block(got_grads, b).double(), pin_block(g_bf16, b).double(), pin_block(g64, b)) for b in blocks]
    pairs += [("V", got_V.double(), info_bf16["V"].double(), info64["V"]),
              ("adv", got_adv.double(), info_bf16["adv"].double(), info64["adv"])]
    if logp is not None:
        pairs.append(("logp",) + tuple(t.double() for t in logp))
    pairs += [(k,) + tuple(t.double() for t in v) for k, v in (extra or {}).items()]
    for name, got, ref, tru in pairs:
        e_hip, e_ref = (got - tru).norm().item(), (ref - tru).norm().item()
        ratios[name] = e_hip / max(e_ref, 1e-300)
        if not e_hip <= (factors or {}).get(name, factor) * e_ref:
            bad.append((name, e_hip, e_ref))
    assert not bad, (bad, ratios)
    return ratios


def trained_like_params(seed):
    """A [NPARAMS] f32 master away from the initial state, where much of the learner's arithmetic
    is degenerate (every bias exactly 0, actor head gain 0.01 so mu ~ 0, one log_std for all 15
    actions): both networks built as PGTrainer._init_params builds them (orthogonal, gain sqrt 2
    on the hidden layers, 1.0 on the value head) but actor head gain 0.5 (log pi of the bf16
    restatement then sits within ~0.02 of fp64; gain 2.0 gives up to 0.13, too close to the clip
    margins of offpolicy_logp), the W1 bias column and b2 ~ U(-0.1, 0.1), b3 ~ U(-0.3, 0.3) on the
    live head rows, log_std = linspace(-1.0, -0.2, 15)."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    params = torch.zeros(NPARAMS, dtype=torch.float32)
    Wd = unpack(params)
    for net, head_rows, head_gain in (("a", ACT, 0.5), ("c", 1, 1.0)):
        for name, r, c, gain in ((f"W1{net}", H, OBS_IN, math.sqrt(2)), (f"W2{net}", H, H, math.sqrt(2)),
                                 (f"W3{net}", head_rows, H, head_gain)):
            w = torch.empty(r, c)
            torch.nn.init.orthogonal_(w, gain=gain, generator=g)
            Wd[name][:r, :c] = w
        u = lambda k, a: (2 * torch.rand(k, generator=g) - 1) * a  # noqa: E731
        Wd[f"W1{net}"][:, OBS_IN] = u(H, 0.1)
        Wd[f"W2{net}"][:, H] = u(H, 0.1)
        Wd[f"W3{net}"][:head_rows, H] = u(head_rows, 0.3)
    Wd["logstd"][:] = torch.linspace(-1.0, -0.2, ACT)
    return params


def clip_bounds(clip_eps):
    """The clip range's boundaries in log-ratio space: (hi, lo) = (log(1 + eps), -log(1 - eps)),
    the ratio being clipped above hi and below -lo."""
    return math.log1p(clip_eps), -math.log1p(-clip_eps)


def offpolicy_logp(logp, clip_eps, seed, band=0.08, reach=0.7, positive=0.65):
    """Old log-probabilities that put the ratio exp(lp - logp_old) on both sides of both clip
    boundaries with a dead band around each: logp + pert, half of the samples with
    |pert| ~ U(0, hi - band) (inside the clip range), the other half with
    |pert| ~ U(lo + band, lo + reach) (outside it; lo > hi, so either sign clears its boundary by
    `band`), signs + for 65 % and - for 35 %, so that approx_kl = mean(pert) is clearly nonzero.
    reach and the sign split are sized by the GPU tests' own input condition |approx_kl| >= 10 x its
    tolerance (2 x the mean |log pi| gap between the bf16 restatement and fp64, 0.0050 on the
    rollout's tapes under trained_like_params): mean(pert) = (2 positive - 1) x mean |pert|, which
    the dead band's width does not move.  reach 0.4 with 60 / 40 gave approx_kl 0.037 (eps 0.1) to
    0.053 (eps 0.2) on those tapes against the 0.050 needed; 0.7 with 65 / 35 gives about 0.075 and
    0.10, while the rarest sign x side combination keeps 0.5 x 0.35 x P(sign A) > 5 % of the samples
    for P(sign A) down to 0.3."""
    hi, lo = clip_bounds(clip_eps)
    assert hi > band and reach > band
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    M = logp.numel()
    u = torch.rand(M, generator=g, dtype=torch.float64)
    outside = torch.rand(M, generator=g) < 0.5
    sign = torch.where(torch.rand(M, generator=g) < positive, 1.0, -1.0).double()
    mag = torch.where(outside, lo + band + u * (reach - band), u * (hi - band))
    pert = (sign * mag).to(logp.dtype).to(logp.device)
    return logp + pert.view_as(logp)


def ratio_margin(info, clip_eps):
    """Smallest distance, in log space, of any sample's ratio (info of loss_and_grads) to either clip
    boundary: above it a computation whose log pi differs from the reference's by less still puts
    every sample on the same side."""
    hi, lo = clip_bounds(clip_eps)
    lr = (info["lp"] - info["logp_old"]).double()
    return torch.minimum((lr - hi).abs(), (lr + lo).abs()).min().item()


def clip_quadrants(info, clip_eps):
    """Fractions of the samples in the four combinations of advantage sign and clipped side:
    {(A > 0, above), (A > 0, below), (A < 0, above), (A < 0, below)}."""
    A, r = info["A"], info["ratio"]
    above, below = r > 1 + clip_eps, r < 1 - clip_eps
    f = lambda m: m.double().mean().item()  # noqa: E731
    return {"A+above": f((A > 0) & above), "A+below": f((A > 0) & below),
            "A-above": f((A < 0) & above), "A-below": f((A < 0) & below)}
