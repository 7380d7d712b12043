"""Restatement of dxrl_pg_popart_rescale and of the forgetting fold (include/dxrl.h), operation for
operation in NumPy float64 (test-only).

The rescale, with (mu_h, sigma_h) the head's pair and (mu_n, sigma_n) the vnorm block's:

    s  = sigma_h / sigma_n
    w' = (float)((double)w * s)                                      256 head weights
    b' = (float)((sigma_h * (double)b + (mu_h - mu_n)) / sigma_n)    the bias

so that sigma_n (w' h + b') + mu_n = sigma_h (w h + b) + mu_h up to the roundings of w' and b'.

The forgetting fold discounts the running (count, M2) with d = 1 - forget and keeps the mean; the
merge and the refresh of (mu, sigma) are pg_vnorm_reference.fold's, imported and not copied.
"""
import math
import struct

import numpy as np

import pg_vnorm_reference as VN

HEAD = 257  # the critic head's row 0: 256 weights, then the bias


def fresh_block():
    """The named words of a fresh popart block."""
    return {"mu_head": 0.0, "sigma_head": 1.0, "rescales": 0.0, "skipped": 0.0, "last_scale": 0.0, "last_shift": 0.0}


def _bits(x):
    return struct.pack("<d", float(x))


def case(mu_h, sigma_h, mu_n, sigma_n):
    """'refused', 'noop' or 'rescale', in the order the header decides them."""
    ok = all(math.isfinite(x) for x in (mu_h, sigma_h, mu_n, sigma_n)) and sigma_h > 0.0 and sigma_n > 0.0
    if not ok:
        return "refused"
    if _bits(mu_h) == _bits(mu_n) and _bits(sigma_h) == _bits(sigma_n):
        return "noop"
    return "rescale"


def rescale_head(head, mu_h, sigma_h, mu_n, sigma_n):
    """head: f32 [257] (weights, bias) -> the rescaled f32 [257], the scale s and the shift."""
    head = np.asarray(head, dtype=np.float32)
    assert head.shape == (HEAD,)
    mu_h, sigma_h, mu_n, sigma_n = (np.float64(x) for x in (mu_h, sigma_h, mu_n, sigma_n))
    s = sigma_h / sigma_n
    out = np.empty(HEAD, dtype=np.float32)
    out[:HEAD - 1] = (head[:HEAD - 1].astype(np.float64) * s).astype(np.float32)
    out[HEAD - 1] = np.float32((sigma_h * np.float64(head[HEAD - 1]) + (mu_h - mu_n)) / sigma_n)
    return out, float(s), float((mu_h - mu_n) / sigma_n)


def vnorm_std(n, m2):
    return math.sqrt(m2 / n) if n > 0.0 else 0.0


def popart_call(head, block, vnorm):
    """One dxrl_pg_popart_rescale call.  head f32 [257]; block: the popart words by name; vnorm: the
    vnorm words by name (_native.PG_VNORM_NAMES).  -> (head', block', row or None): row is the
    dict of dxrl_pg_vnorm_log_col, None on a refusal (nothing but SKIPPED is written)."""
    mu_h, sigma_h, mu_n, sigma_n = block["mu_head"], block["sigma_head"], vnorm["mu"], vnorm["sigma"]
    what = case(mu_h, sigma_h, mu_n, sigma_n)
    out = dict(block)
    if what == "refused":
        out["skipped"] += 1.0
        return np.array(head, dtype=np.float32), out, None
    if what == "noop":
        new, s, shift = np.array(head, dtype=np.float32), 1.0, 0.0
    else:
        new, s, shift = rescale_head(head, mu_h, sigma_h, mu_n, sigma_n)
        out.update(mu_head=mu_n, sigma_head=sigma_n, rescales=block["rescales"] + 1.0, last_scale=s, last_shift=shift)
    row = {"mu": mu_n, "sigma": sigma_n, "mu_prev": mu_h, "sigma_prev": sigma_h, "scale": s, "shift": shift,
           "rescaled": 0.0 if what == "noop" else 1.0, "count": vnorm["count"], "mean": vnorm["mean"],
           "std": vnorm_std(vnorm["count"], vnorm["m2"]), "batch_mean": vnorm["batch_mean"],
           "batch_std": vnorm_std(vnorm["batch_count"], vnorm["batch_m2"]), "calls": vnorm["calls"],
           "forget": vnorm["forget"]}
    return new, out, row


def decoded(head, h, mu, sigma):
    """sigma (w h + b) + mu in f64 for hidden rows h [rows][256]."""
    head = np.asarray(head, dtype=np.float64)
    return sigma * (np.asarray(h, dtype=np.float64) @ head[:HEAD - 1] + head[HEAD - 1]) + mu


def preservation_bound(head, mu_h, sigma_h, mu_n):
    """The derived bound on |decoded after - decoded before| through a bf16 pack of the head, for
    hidden units in [-1, 1] (tanh): both packs round each head weight to bf16 (relative 2^-9 each,
    2^-8 together), and the f32 roundings of w', b' and the decode get a slack of 8 ulps of the
    terms' magnitudes."""
    head = np.asarray(head, dtype=np.float64)
    sw, b = np.abs(head[:HEAD - 1]).sum(), abs(head[HEAD - 1])
    return 2.0 ** -8 * sigma_h * sw + 8.0 * 2.0 ** -24 * (abs(mu_h) + abs(mu_n) + sigma_h * (sw + b))


def fold_forget(state, batch, eps, forget):
    """pg_vnorm_reference.fold behind the discount: count <- d count, M2 <- d M2 with d = 1 - forget
    (the mean kept), then the merge and the refresh as they are."""
    d = 1.0 - float(forget)
    n, mean, m2 = state["running"]
    return VN.fold(dict(state, running=(d * n, mean, d * m2)), batch, eps)


def weighted_moments(batches, forget):
    """The explicitly weighted two-pass (count, mean, M2) after folding `batches` (1-d arrays) in
    order: an element of batch i of k carries the weight (1 - forget) ** (k - 1 - i)."""
    k = len(batches)
    x = np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1) for b in batches])
    w = np.concatenate([np.full(np.asarray(b).size, (1.0 - forget) ** (k - 1 - i)) for i, b in enumerate(batches)])
    n = w.sum()
    mean = (w * x).sum() / n
    return float(n), float(mean), float((w * (x - mean) ** 2).sum())
