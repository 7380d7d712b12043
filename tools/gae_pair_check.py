"""Every output buffer of the three GAE entry points (dxrl_pg_gae, dxrl_pg_gae_timelimit,
dxrl_pg_gae_vnorm with both tapes) on seeded inputs, saved whole to ab_out/gpc_<TAG>.pt, so
two kernel libraries (DXRL_LIB) can be compared bit for bit, the moments included:
python tools/gae_pair_check.py TAG  /  python tools/gae_pair_check.py --compare TAG_A TAG_B.

Envs: a lone env, one full k_gae_lds group, a ragged second group, three groups, a second k_gae
wave.  Horizons: no full chunk (1), one 8-step chunk and one step more, 15 / 16 / 17 chunks (a
segment per lane, one more), the last horizon staged in LDS and the first of the k_gae fallback;
and the workload's 4096 x 200.  Ends at 5 % of the steps, time limits and terminations alike.
The value-normalisation form runs three calls per tape: on a fresh block, on a prepared block
(running moments, constants and a forgetting factor set) and, on that block, without the fold."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = [(n, T) for n in (1, 16, 17, 40, 65) for T in (1, 8, 9, 120, 128, 136, 600, 601)] + [(4096, 200)]
GAMMA, LAM, EPS = 0.99, 0.95, 1e-8
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ab_out")


def bits(t):
    """The tensor's bits as integers: -0.0 differs from 0.0 and a NaN equals itself."""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


if len(sys.argv) < 2 or (sys.argv[1] == "--compare" and len(sys.argv) < 4):
    sys.exit(__doc__)
if sys.argv[1] == "--compare":
    a, b = (torch.load(os.path.join(OUT, f"gpc_{t}.pt"), weights_only=True) for t in sys.argv[2:4])
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not torch.equal(bits(a[k]), bits(b[k]))]
    print(f"{len(a)} buffers of {len(SIZES)} shapes:", "bit-identical" if not bad else f"DIFFER at {bad}", flush=True)
    sys.exit(1 if bad else 0)

from dexterous_rl_manipulation_amd import _native as N  # noqa: E402

dev = torch.device("cuda:0")
res = {}


def inputs(n, T):
    g = torch.Generator().manual_seed(1000 * n + T)
    rew = torch.randn(T * n, generator=g) + 1.0
    V = torch.randn((T + 1) * n, generator=g)
    ends = torch.rand(T * n, generator=g) < 0.05
    lengths = torch.randint(1, 1 << 15, (T * n,), generator=g)
    kind = torch.randint(0, 2, (T * n,), generator=g)
    codes = torch.where(ends, (lengths << 1) | kind, torch.zeros_like(lengths))
    code16 = torch.from_numpy(codes.numpy().astype(np.uint16).view(np.int16))
    return rew.to(dev), V.to(dev), {"done": ends.to(torch.uint8).to(dev), "ep_code": code16.to(dev)}


def outputs(n, T, partial_doubles, tape):
    o = {k: torch.zeros(T * n, device=dev) for k in ("adv", "ret", "ret_norm")}
    o["values_raw"] = torch.zeros((T + 1) * n, device=dev)
    o["partial"] = torch.zeros(partial_doubles, dtype=torch.float64, device=dev)
    o["stats"] = torch.zeros(8, dtype=torch.float64, device=dev)
    if tape == "ep_code":
        o["counts"] = torch.zeros(N.gae_timelimit_count_words(n, T), dtype=torch.int64, device=dev)
    return o


def keep(tag, o):
    torch.cuda.synchronize()
    for k, v in o.items():
        res[f"{tag}/{k}"] = v.cpu().clone()


def prepared_block():
    block = N.vnorm_fresh(None)
    for k, v in (("count", 8000.0), ("mean", 34.123456789), ("m2", 8000.0 * 120.5), ("mu", float(np.float32(34.1))),
                 ("sigma", float(np.float32(10.9))), ("calls", 5.0), ("eps", EPS), ("forget", 0.125)):
        block[N.PG_VNORM[k]] = v
    return block.to(dev)


for n, T in SIZES:
    rew, V, tapes = inputs(n, T)
    for tape, entry in (("done", "dxrl_pg_gae"), ("ep_code", "dxrl_pg_gae_timelimit")):
        o = outputs(n, T, N.gae_partial_doubles(n, T), tape)
        del o["ret_norm"], o["values_raw"]
        tail = [N.ptr(o["counts"])] if tape == "ep_code" else []
        N.call(entry, 0, N.ptr(rew), N.ptr(tapes[tape]), N.ptr(V), n, T, GAMMA, LAM, N.ptr(o["adv"]), N.ptr(o["ret"]),
               N.ptr(o["partial"]), N.ptr(o["stats"]), *tail, N.stream_of(dev))
        keep(f"{n}x{T}/{entry}", o)
        for call, fold in (("fresh", 1), ("prepared", 1), ("unfolded", 0)):
            if call != "unfolded":
                block = N.vnorm_fresh(dev) if call == "fresh" else prepared_block()
            o = outputs(n, T, N.gae_vnorm_partial_doubles(n, T), tape)
            a = N.PgGaeVnormArgs()
            a.rew, a.values = N.ptr(rew), N.ptr(V)
            if tape == "ep_code":
                a.ep_code, a.counts = N.ptr(tapes[tape]), N.ptr(o["counts"])
            else:
                a.done = N.ptr(tapes[tape])
            a.num_envs, a.horizon, a.gamma, a.lam, a.eps = n, T, GAMMA, LAM, EPS
            a.adv, a.ret, a.ret_norm, a.values_raw = (N.ptr(o[k]) for k in ("adv", "ret", "ret_norm", "values_raw"))
            a.partial, a.stats, a.vnorm, a.fold = N.ptr(o["partial"]), N.ptr(o["stats"]), N.ptr(block), fold
            N.call("dxrl_pg_gae_vnorm", 0, C.byref(a), N.stream_of(dev))
            o["vnorm"] = block
            keep(f"{n}x{T}/dxrl_pg_gae_vnorm/{tape}/{call}", o)
os.makedirs(OUT, exist_ok=True)
torch.save(res, os.path.join(OUT, f"gpc_{sys.argv[1]}.pt"))
print(sys.argv[1], os.path.basename(N.LIB_PATH), len(res), "buffers of", len(SIZES), "shapes saved", flush=True)
