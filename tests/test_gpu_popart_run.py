"""GPU: TrainerConfig.popart and value_norm_forget at run level -- 64 envs x 40 steps on the hard
curriculum with an episode limit of 8 steps (the setting of tests/test_gpu_vnorm_run.py): the
iteration is the value_norm trainer's up to its last optimiser step, then the head moves into the
new units and the decoded values stay; the log table, the checkpoints and two sharded ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pg_popart_reference as PA
import pg_vnorm_reference as VN
import test_gpu_vnorm_run as VR  # its setting and helpers: make, make_env, same, _port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TAPES = VR.TAPES
FORGET = 0.05
WAIT_S = 240


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import envs, trainer  # noqa: F401
    return d


@pytest.fixture(scope="module")
def N():
    from dexterous_rl_manipulation_amd import _native
    return _native


def head_of(pkg, params):
    lo = pkg.trainer.OFF["W3c"]
    return params[lo:lo + PA.HEAD].cpu().numpy()


def repacked(N, tr):
    out = torch.zeros_like(tr.packed)
    N.call("dxrl_pg_pack_weights", 0, N.ptr(tr.params), N.ptr(out), N.stream_of(tr.dev))
    torch.cuda.synchronize()
    return out


def vnorm_words(N, tr):
    b = tr.vnorm.tolist()
    return {k: b[i] for k, i in N.PG_VNORM.items()}


def popart_words(N, tr):
    b = tr.popart.tolist()
    return {k: b[i] for k, i in N.PG_POPART.items()}


@pytest.mark.parametrize("fused", [True, False])
def test_two_iterations_against_the_value_norm_trainer(pkg, N, fused):
    """Iteration 0: every buffer the iteration writes up to and including the last optimiser step is
    the value_norm trainer's bit for bit; afterwards the head is the restatement's rescale of that
    trainer's head from the fresh pair into the folded one, the pack is dxrl_pg_pack_weights of the
    new master, and everything else is equal.
    Iteration 1 (update=False): V_raw = sigma_1 vn' + mu_1 agrees with the un-rescaled weights'
    values in their own units (the value_norm trainer's critic output on the same observations,
    decoded with the fresh pair) within the derived bound; that trainer's own V_raw, decoded with
    the moved pair, is off by more than the bound.  The iteration rescales again."""
    _, vn = VR.make(pkg, value_norm=True, fused=fused)
    _, pa = VR.make(pkg, value_norm=True, popart=True, fused=fused)
    assert vn.popart is None and pa.popart is not None
    with pytest.raises(ValueError, match="popart"):
        vn.popart_state()
    vn.iteration()
    pa.iteration()
    torch.cuda.synchronize()
    for name in TAPES + ("adv", "ret", "ret_norm", "V_raw", "stats", "grads", "m1", "m2", "vnorm"):
        assert VR.same(getattr(pa, name), getattr(vn, name)), name
    assert VR.same(pa.V[0], vn.V[0])
    w = vnorm_words(N, pa)
    assert (w["mu"], w["sigma"]) != (0.0, 1.0)  # a condition on the input: the pair moved
    head0 = head_of(pkg, vn.params)
    want_head, want_block, _ = PA.popart_call(head0, PA.fresh_block(), w)
    assert head_of(pkg, pa.params).tobytes() == want_head.tobytes()
    assert head_of(pkg, pa.params).tobytes() != head0.tobytes()
    expect = vn.params.clone()
    lo = pkg.trainer.OFF["W3c"]
    expect[lo:lo + PA.HEAD] = torch.from_numpy(want_head).to(expect.device)
    assert VR.same(pa.params, expect)
    assert VR.same(pa.packed, repacked(N, pa)) and VR.same(vn.packed, repacked(N, vn))
    assert popart_words(N, pa) == want_block
    state = pa.popart_state()
    assert state == {"mu_head": w["mu"], "sigma_head": w["sigma"], "rescales": 1, "skipped": 0,
                     "last_scale": want_block["last_scale"], "last_shift": want_block["last_shift"]}

    vn.iteration(update=False)
    pa.iteration(update=False)
    torch.cuda.synchronize()
    for name in TAPES:
        assert VR.same(getattr(pa, name), getattr(vn, name)), name
    bound = PA.preservation_bound(head0, 0.0, 1.0, w["mu"])
    own_units = vn.V[0].double().cpu().numpy()  # the un-rescaled head under the pair it was trained with
    err = np.abs(pa.V_raw.double().cpu().numpy() - own_units).max()
    # (the median: a single value may sit where (sigma_1 - 1) vn + mu_1 crosses zero)
    jump = np.median(np.abs(vn.V_raw.double().cpu().numpy() - own_units))
    print(f"fused={fused}: popart V_raw off by at most {err:.3e}, bound {bound:.3e}; value_norm V_raw off by "
          f"{jump:.3e} (median); (mu, sigma) = ({w['mu']:.6g}, {w['sigma']:.6g})")
    assert err <= bound
    assert jump > bound
    # the un-updated iteration folded again, and its rescale took the head on
    w1 = vnorm_words(N, pa)
    # (the two trainers' moments part here: the value_norm trainer's returns came from jumped values)
    assert (w1["mu"], w1["sigma"]) != (w["mu"], w["sigma"]) and not VR.same(pa.vnorm, vn.vnorm)
    again, block1, _ = PA.popart_call(want_head, want_block, w1)
    assert head_of(pkg, pa.params).tobytes() == again.tobytes() and popart_words(N, pa) == block1
    assert pa.popart_state()["rescales"] == 2 and VR.same(pa.packed, repacked(N, pa))
    assert VR.same(pa.m1, vn.m1) and VR.same(pa.m2, vn.m2)  # Adam's moments are left alone


def test_ppo_passes_with_bootstrap_and_a_kl_rule(pkg):
    _, tr = VR.make(pkg, value_norm=True, popart=True, value_norm_forget=FORGET, timeout_bootstrap=True, epochs=2,
                    minibatches=2, target_kl=0.02)
    log = tr.fit(2)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.params).all() and np.isfinite(log["value_mse"]).all()
    assert tr.popart_state()["rescales"] == 2 and tr.popart_state()["skipped"] == 0
    assert log.optimizer is not None and len(log.value_norm) == 2 and (log.value_norm["rescaled"] == 1.0).all()
    for bad in (dict(popart=True), dict(value_norm_forget=0.1), dict(value_norm=True, value_norm_forget=1.0)):
        with pytest.raises(ValueError, match="popart|value_norm_forget"):
            VR.make(pkg, **bad)


def test_fit_writes_the_value_norm_table_row_by_row(pkg, N):
    from dexterous_rl_manipulation_amd import training_run as T
    _, tr = VR.make(pkg, value_norm=True, popart=True, value_norm_forget=FORGET)
    prev = (0.0, 1.0)
    for k in range(3):
        log = tr.fit(1)
        torch.cuda.synchronize()
        assert len(log) == k + 1 and len(log.value_norm) == k + 1
        row = {name: log.value_norm[name][k] for name in T.VNORM_COLUMNS}
        p, v = tr.popart_state(), tr.value_norm_state()
        assert (row["mu"], row["sigma"]) == (v["mu"], v["sigma"]) == (p["mu_head"], p["sigma_head"])
        assert (row["mu_prev"], row["sigma_prev"]) == prev
        assert (row["scale"], row["shift"], row["rescaled"]) == (p["last_scale"], p["last_shift"], 1.0)
        assert row["scale"] == prev[1] / row["sigma"] and row["shift"] == (prev[0] - row["mu"]) / row["sigma"]
        assert (row["count"], row["mean"], row["std"]) == (v["count"], v["mean"], v["std"])
        assert (row["batch_mean"], row["batch_std"], row["calls"]) == (v["batch_mean"], v["batch_std"], k + 1)
        assert row["forget"] == FORGET and p["rescales"] == k + 1
        prev = (row["mu"], row["sigma"])
    # the discounted count: M, then (1 - f) M + M, ...
    assert log.value_norm["count"].tolist() == [tr.M, (1 - FORGET) * tr.M + tr.M,
                                               (1 - FORGET) * ((1 - FORGET) * tr.M + tr.M) + tr.M]
    back = T.TrainingLog.from_dict(log.to_dict())
    assert back.value_norm.table.tobytes() == log.value_norm.table.tobytes()
    assert back.table.tobytes() == log.table.tobytes()
    plain = VR.make(pkg, value_norm=True)[1].fit(1)
    assert plain.value_norm is None and "value_norm" not in plain.to_dict()


def test_resumed_run_continues_bit_for_bit(pkg, tmp_path):
    kw = dict(value_norm=True, popart=True, value_norm_forget=FORGET)
    _, whole = VR.make(pkg, **kw)
    log_w = whole.fit(4)
    _, a = VR.make(pkg, **kw)
    a.fit(2)
    path = tmp_path / "ck.npz"
    a.save_checkpoint(path)
    r = pkg.trainer.PGTrainer.load_checkpoint(path, VR.make_env(pkg))
    assert r.cfg == a.cfg and r.cfg.popart and r.cfg.value_norm_forget == FORGET
    assert VR.same(r.vnorm, a.vnorm) and VR.same(r.popart, a.popart)
    log_r = r.fit(2)
    torch.cuda.synchronize()
    for name in ("params", "m1", "m2", "packed", "adv", "ret", "ret_norm", "V_raw", "vnorm", "popart"):
        assert VR.same(getattr(whole, name), getattr(r, name)), name
    assert len(log_r) == 4 and log_r.table.tobytes() == log_w.table.tobytes() and log_r.header == log_w.header
    assert log_r.value_norm.table.tobytes() == log_w.value_norm.table.tobytes()
    assert whole.popart_state() == r.popart_state() and r.popart_state()["rescales"] == 4


def test_older_checkpoints_load_and_mismatches_raise(pkg, tmp_path):
    """A value_norm trainer writes the file it always did (no popart field, no block, no table) and
    loads with popart False and a forgetting factor of 0; a file whose popart block and field
    disagree raises naming popart; a vnorm block whose FORGET word disagrees with the configuration
    raises naming value_norm_forget."""
    from dexterous_rl_manipulation_amd import _native as N
    from dexterous_rl_manipulation_amd import training_run as T
    _, old = VR.make(pkg, value_norm=True)
    old.fit(1)
    old.save_checkpoint(tmp_path / "old.npz")
    arrays_o, meta_o = T.read_checkpoint(tmp_path / "old.npz")
    assert "popart" not in meta_o["trainer_config"] and "value_norm_forget" not in meta_o["trainer_config"]
    assert "popart_state" not in arrays_o and "log_value_norm" not in arrays_o
    r = pkg.trainer.PGTrainer.load_checkpoint(tmp_path / "old.npz", VR.make_env(pkg))
    assert r.cfg.popart is False and r.cfg.value_norm_forget == 0.0 and r.popart is None
    r.iteration()
    _, opt = VR.make(pkg, value_norm=True, popart=True, value_norm_forget=FORGET)
    opt.fit(1)
    opt.save_checkpoint(tmp_path / "opt.npz")
    arrays, meta = T.read_checkpoint(tmp_path / "opt.npz")
    assert meta["trainer_config"]["popart"] is True and meta["trainer_config"]["value_norm_forget"] == FORGET
    assert arrays["popart_state"].shape == (N.PG_POPART_WORDS,)
    assert arrays["log_value_norm"].shape == (1, N.PG_VNORM_LOG_COLS)
    assert arrays["value_norm_state"][N.PG_VNORM["forget"]] == FORGET

    def refused(name, match, arrays, meta):
        T.write_checkpoint(tmp_path / name, arrays, meta)
        with pytest.raises(ValueError, match=match):
            pkg.trainer.PGTrainer.load_checkpoint(tmp_path / name, VR.make_env(pkg))

    cfg = meta["trainer_config"]
    refused("block_only.npz", "popart", arrays, dict(meta, trainer_config={k: v for k, v in cfg.items() if k != "popart"}))
    refused("field_only.npz", "popart", {k: v for k, v in arrays.items() if k != "popart_state"}, meta)
    refused("forget_field.npz", "value_norm_forget", arrays, dict(meta, trainer_config=dict(cfg, value_norm_forget=0.25)))
    refused("forget_none.npz", "value_norm_forget", arrays,
            dict(meta, trainer_config={k: v for k, v in cfg.items() if k != "value_norm_forget"}))
    torch.cuda.synchronize()


def test_one_rescale_launch_per_iteration_and_none_without_the_option(pkg, N, monkeypatch):
    calls = []
    real = N.call

    def recorder(name, *args):
        calls.append(name)
        return real(name, *args)

    _, vn = VR.make(pkg, value_norm=True)
    _, pa = VR.make(pkg, value_norm=True, popart=True)
    _, plain = VR.make(pkg)
    monkeypatch.setattr(N, "call", recorder)
    for tr in (vn, plain):
        tr.iteration()
        tr.iteration(update=False)
        tr.fit(1)
    assert calls and "dxrl_pg_popart_rescale" not in calls
    del calls[:]
    pa.iteration()
    assert calls.count("dxrl_pg_popart_rescale") == 1 and calls[-1] == "dxrl_pg_popart_rescale"
    pa.iteration(update=False)
    pa.fit(2)
    torch.cuda.synchronize()
    assert calls.count("dxrl_pg_popart_rescale") == 4


def launch(tmp, world, n):
    """Start `world` ranks of tests/sharded_popart_worker.py and wait for each with a timeout; on
    any failure or timeout every remaining rank is killed before the assertion.  No retries."""
    port = VR._port()
    procs, outs = [], []
    for r in range(world):
        out = os.path.join(tmp, f"popart_w{world}_r{r}.pt")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "sharded_popart_worker.py"), out, str(n)],
                                      env=env))
        outs.append(out)
    codes = []
    try:
        for p in procs:
            codes.append(p.wait(timeout=WAIT_S))
            if codes[-1] != 0:
                break
    except subprocess.TimeoutExpired:
        codes.append("timeout")
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    assert codes == [0] * world, codes
    return [torch.load(o, weights_only=False) for o in outs]


def test_two_ranks_end_with_identical_weights_and_blocks(pkg, tmp_path):
    """World 2 over gloo on one GPU, 32 envs per rank, two iterations with a forgetting factor:
    params, packed and both state blocks are byte-identical on the ranks; each rank rescaled twice
    into the pair its vnorm block holds."""
    from dexterous_rl_manipulation_amd import _native as N
    world, n = 2, VR.N_ENVS // 2
    a, b = launch(str(tmp_path), world, n)
    for key in ("params", "packed", "vnorm", "popart"):
        assert VR.same(a[key], b[key]), key
    assert a["popart_state"] == b["popart_state"] and a["popart_state"]["rescales"] == 2
    assert a["popart_state"]["skipped"] == 0
    assert (a["popart_state"]["mu_head"], a["popart_state"]["sigma_head"]) == \
        (a["value_norm_state"]["mu"], a["value_norm_state"]["sigma"])
    M = VR.N_ENVS * VR.HORIZON
    assert a["vnorm"][N.PG_VNORM["forget"]] == 0.05 and a["value_norm_state"]["count"] == (1 - 0.05) * M + M
