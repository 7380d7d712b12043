"""GPU: dxrl_pg_gae_timelimit (csrc/dxrl_pg_gae.hip, k_gae_lds<true, false> / k_gae<true, false>) through ctypes
against its restatement (tests/pg_timelimit_reference.py), at the smallest shapes that reach each
code path of the two kernels."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import pg_reference as R
import pg_timelimit_reference as TL

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.95
# k_gae_lds: one chunk with 15 empty segments (1, 8), a chunk boundary (9), fewer chunks than the
# 16 segments (120), exactly 16 chunks (128), one more (136), the workload's horizon (200);
# a lone env, one full workgroup, a partial second one, three (the XCD group permutation)
LDS_T = (1, 8, 9, 120, 128, 136, 200)
LDS_N = (1, 16, 17, 40)
# k_gae: the first horizon whose staging no longer fits the LDS; a lone env, a full wave, one more
SEQ_T = next(T for T in itertools.count(1) if not R.gae_uses_segmented_scan(T))
SEQ_N = (1, 64, 65)
CASES = ([(n, T) for T in LDS_T for n in LDS_N] + [(17, SEQ_T - 1)]  # the largest staged horizon
         + [(n, SEQ_T) for n in SEQ_N])
CANARY = 64


@pytest.fixture(scope="module")
def N():
    from dexterous_rl_manipulation_amd import _native
    return _native


def u16(codes):
    """An integer tensor of values 0 .. 65535 as the int16 tensor holding those u16 bits."""
    return torch.from_numpy(codes.numpy().astype(np.uint16).view(np.int16))


def timeout_at(n, T, steps):
    code = torch.zeros(T, n, dtype=torch.int64)
    for t in steps:
        code[t] = 2 * (t + 1)  # bit 0 clear: a time limit
    return code.reshape(-1)


def tapes(n, T, g):
    """name -> u16 codes [T n] (as int64)."""
    ends = torch.rand(T * n, generator=g) < 0.1
    lengths = torch.randint(1, 1 << 15, (T * n,), generator=g)  # every 15-bit length: codes up to 0xFFFF
    kind = torch.randint(0, 2, (T * n,), generator=g)
    zero = torch.zeros(T * n, dtype=torch.int64)
    out = {"none": zero,
           "terminations": torch.where(ends, (lengths << 1) | 1, zero),
           "mixed": torch.where(ends, (lengths << 1) | kind, zero),
           "timeout_every_step": torch.full((T * n,), 2)}
    # single time limits: first and last step, and both sides of segment boundaries of the scan
    # (lane s of an env owns the 8-step chunks [s nc / 16, (s + 1) nc / 16))
    nc = (T + 7) // 8
    singles = {0, T - 1}
    for s in (1, 8, 15):
        k = s * nc // 16
        if 0 < 8 * k < T:
            singles |= {8 * k - 1, 8 * k}
    for t in sorted(singles):
        out[f"timeout_at_{t}"] = timeout_at(n, T, [t])
    return out


def run(N, name, rew, tape, V, n, T, gamma=GAMMA, lam=LAM):
    """(adv, ret, stats, counts) of dxrl_pg_gae_timelimit / dxrl_pg_gae with NaN / -7 canaries
    behind the sized scratch."""
    dev = rew.device
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    need = N.gae_partial_doubles(n, T)
    part = torch.full((need + CANARY,), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    args = [0, N.ptr(rew), N.ptr(tape), N.ptr(V), n, T, gamma, lam, N.ptr(adv), N.ptr(ret), N.ptr(part), N.ptr(stats)]
    counts = None
    if name == "dxrl_pg_gae_timelimit":
        words = N.gae_timelimit_count_words(n, T)
        assert words == 2 + 2 * ((n + 15) // 16)
        counts = torch.full((words + CANARY,), -7, dtype=torch.int64, device=dev)
        args.append(N.ptr(counts))
    N.call(name, *args, N.stream_of(dev))
    torch.cuda.synchronize()
    assert torch.isnan(part[need:]).all(), f"{name} wrote past dxrl_pg_gae_partial_doubles"
    if counts is not None:
        assert (counts[words:] == -7).all(), f"{name} wrote past dxrl_pg_gae_timelimit_count_words"
        counts = counts[:words]
    return adv, ret, stats, counts


@pytest.mark.parametrize("n,T", CASES)
def test_timelimit_gae_matches_restatement(N, n, T):
    """adv / ret bit for bit the restatement's on every tape; on the tapes without a time limit
    also dxrl_pg_gae's own output on the matching done bytes; stats within the bounds
    tests/test_gpu_pg.py holds dxrl_pg_gae to; counts exact.  rew ~ N(0, 1), V ~ N(0, 50): a
    wrong bootstrap is far outside rounding."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(n * 1000 + T)
    rew_h = torch.randn(T * n, generator=g)
    V_h = torch.randn((T + 1) * n, generator=g) * 50.0
    rew, V = rew_h.to(dev), V_h.to(dev)
    assert R.gae_uses_segmented_scan(T) == (T < SEQ_T)
    seen = set()
    for name, code in tapes(n, T, g).items():
        a_ref, r_ref = TL.gae_timelimit(rew_h, code, V_h, n, T, GAMMA, LAM)
        adv, ret, stats, counts = run(N, "dxrl_pg_gae_timelimit", rew, u16(code).to(dev), V, n, T)
        assert torch.equal(adv.cpu(), a_ref) and torch.equal(ret.cpu(), r_ref), name
        timeouts, terminations = TL.end_counts(code)
        assert counts[:2].tolist() == [timeouts, terminations], name
        # one pair per launched workgroup: 16 envs each in k_gae_lds, 64 in k_gae
        pairs = counts[2:2 + 2 * (-(-n // (16 if T < SEQ_T else 64)))]
        assert pairs[0::2].sum().item() == timeouts and pairs[1::2].sum().item() == terminations, name
        a = adv.double()
        assert stats[0].item() == n * T, name
        assert math.isclose(stats[2].item(), a.mean().item(), rel_tol=1e-9, abs_tol=1e-12), name
        if n * T > 1:
            assert math.isclose(stats[4].item(), a.std().item(), rel_tol=1e-9), name
        if timeouts == 0:  # the cross-check that needs no restatement
            done = (code != 0).to(torch.uint8).to(dev)
            a_gae, r_gae, s_gae, _ = run(N, "dxrl_pg_gae", rew, done, V, n, T)
            assert torch.equal(adv, a_gae) and torch.equal(ret, r_gae) and torch.equal(stats, s_gae), name
        else:
            # and the restatement's bootstrap is the intended one: at a time limit, where the chain
            # stops, A is the plain GAE's plus gamma V_t (each A three roundings of numbers below
            # ~500: 6 x 2^-24 x 500 < 2e-4; gamma |V_t| is of order 50)
            a_plain, _ = R.gae(rew_h, (code != 0).to(torch.uint8), V_h, n, T, GAMMA, LAM)
            lim = TL.end_masks(code)[2]
            assert ((a_ref - a_plain)[lim] - GAMMA * V_h[:T * n][lim]).abs().max().item() < 1e-3, name
        seen.add((timeouts > 0, terminations > 0))
    assert {(False, False), (True, False)} <= seen and (n * T < 40 or {(False, True), (True, True)} <= seen)


def test_invalid_arguments_leave_outputs_untouched(N):
    """A null pointer, num_envs < 1 or horizon < 1: DXRL_E_INVALID before any launch."""
    dev = torch.device("cuda", 0)
    n, T = 17, 9
    rew, V = torch.randn(T * n, device=dev), torch.randn((T + 1) * n, device=dev)
    code = torch.zeros(T * n, dtype=torch.int16, device=dev)
    adv, ret = torch.full((T * n,), 3.0, device=dev), torch.full((T * n,), 4.0, device=dev)
    part = torch.full((N.gae_partial_doubles(n, T),), 5.0, dtype=torch.float64, device=dev)
    stats = torch.full((8,), 6.0, dtype=torch.float64, device=dev)
    counts = torch.full((N.gae_timelimit_count_words(n, T),), -7, dtype=torch.int64, device=dev)
    good = [0, N.ptr(rew), N.ptr(code), N.ptr(V), n, T, GAMMA, LAM, N.ptr(adv), N.ptr(ret), N.ptr(part), N.ptr(stats),
            N.ptr(counts), N.stream_of(dev)]
    fn = N.lib().dxrl_pg_gae_timelimit
    bad = [(k, None) for k in (1, 2, 3, 8, 9, 10, 11, 12)] + [(4, 0), (4, -1), (5, 0), (5, -3)]
    for k, v in bad:
        args = list(good)
        args[k] = v
        assert fn(*args) == N.DXRL_E_INVALID, (k, v)
        with pytest.raises(ValueError):
            N.call("dxrl_pg_gae_timelimit", *args)
    torch.cuda.synchronize()
    assert (adv == 3.0).all() and (ret == 4.0).all() and (part == 5.0).all() and (stats == 6.0).all()
    assert (counts == -7).all()
    out = C.c_int64(-1)
    for a, b, p in ((0, 5, C.byref(out)), (5, 0, C.byref(out)), (5, 5, None)):
        assert N.lib().dxrl_pg_gae_timelimit_count_words(a, b, p) == N.DXRL_E_INVALID
    assert out.value == -1
    assert fn(*good) == N.DXRL_OK  # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert counts[:2].tolist() == [0, 0] and not (adv == 3.0).all()
