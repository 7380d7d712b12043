"""Restatement of dxrl_pg_gae_timelimit (include/dxrl.h), operation for operation (test-only).

The tape is the rollout's u16 episode-end code in place of the done byte.  Per sample, in f32:

    end = code != 0, term = code & 1, timeout = end and not term
    vb = V_t if timeout else V_{t+1};  nb = 0 if term else 1
    delta_t = r_t + gamma * vb * nb - V_t;  c_t = 0 if end else gamma * lambda
    A_t = delta_t + c_t * A_{t+1};  ret_t = A_t + V_t

delta and c are built here; the scans over them are pg_reference's own (the segmented wavefront
order of k_gae_lds and the one-chain loop of k_gae), imported and not copied: pg_reference.gae
composes delta and c from (rew, done, V) in exactly the operations

    delta_t = rew_t + gamma * V_{t+1} * (1 - done_t) - V_t,   c_t = 0 if done_t else gamma * lambda

so it is handed a `rew`, a `done` and a `V` whose composition gives this module's delta and c
bit for bit: done = end; V = 0 everywhere (gamma * 0 * nd = +0, x + 0 = x and x - 0 = x are
exact, and x + 0 keeps x's sign except for x = -0, which compares equal to +0 and which the tests'
inputs do not produce); rew = delta.  The advantages come out of the scan; ret = A + V is taken
here with the real V."""
import torch

import pg_reference as R


def end_masks(code):
    """(end, term, timeout) boolean masks of a u16 code tape (any integer tensor)."""
    code = code.to(torch.int64) & 0xFFFF
    end = code != 0
    term = (code & 1) != 0
    return end, term, end & ~term


def delta_and_c(rew, code, V, n, T, gamma, lam):
    """f32 delta [T n] and chain coefficient c [T n] of the rule above."""
    rew, V = rew.view(T, n), V.view(T + 1, n)
    end, term, timeout = (m.view(T, n) for m in end_masks(code))
    dt = rew.dtype
    g = torch.tensor(gamma, dtype=dt)
    gl = g * torch.tensor(lam, dtype=dt)
    vb = torch.where(timeout, V[:T], V[1:])
    nb = torch.where(term, torch.zeros((), dtype=dt, device=rew.device), torch.ones((), dtype=dt, device=rew.device))
    delta = rew + g * vb * nb - V[:T]
    c = torch.where(end, torch.zeros((), dtype=dt, device=rew.device), gl.to(rew.device))
    return delta, c


def gae_timelimit(rew, code, V, n, T, gamma, lam, scan=None):
    """rew [T*n] f32, code [T*n] u16 (any integer dtype), V [(T+1)*n] -> adv, ret [T*n].
    scan: as pg_reference.gae (None: the kernel's choice for T; True the segmented scan of
    k_gae_lds, False k_gae's sequential chain)."""
    delta, _ = delta_and_c(rew, code, V, n, T, gamma, lam)
    end = end_masks(code)[0].to(torch.uint8)
    zero_v = torch.zeros((T + 1) * n, dtype=rew.dtype, device=rew.device)
    adv, _ = R.gae(delta.reshape(-1), end.reshape(-1), zero_v, n, T, gamma, lam, scan=scan)
    ret = adv + V.view(-1)[:T * n]
    return adv, ret


def end_counts(code):
    """(time limits, terminations) on the tape."""
    _, term, timeout = end_masks(code)
    return int(timeout.sum()), int(term.sum())
