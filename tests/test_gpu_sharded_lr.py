"""GPU, multi-rank: step-size control on sharded trainers (processes on cuda:0 over gloo, started as
tests/test_gpu_sharded_fit.py starts them: at most 4 ranks at once, a timeout per rank, the remaining
ranks killed on failure, no retries).  256 global envs, horizon 32, episodes capped at 40 steps, PPO
2 epochs x 2 minibatches, 3 iterations.

Every rank merges the same gathered (kl_sum, rows) records in the same order, so master, moments,
pack, the controller's state block, log.optimizer and the training table must be byte-equal across
ranks.  Against the world-1 run on the same 256 envs only row 0's kl_max is comparable (pass 0 runs
on the first rollout's tapes, bit-identical when sharded; afterwards the parameters drift by f32
reduction order): it is held to 1e-4 max(1, |ref|), the bound tests/test_gpu_sharded_fit.py holds the
loss columns to and tests/test_gpu_dist.py the global moments and the all-reduced gradient -- loose
for a KL, which is far below 1; no new number is introduced for it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pg_lr_reference as R
import sharded_lr_worker as K
from test_gpu_sharded_fit import GLOBAL_ENVS, WAIT_S, _port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAME = ("params", "m1", "m2", "packed", "opt_state", "optimizer", "table")
COL = {k: i for i, k in enumerate(R.COLUMNS)}


def launch(tmp, world, mode, arg, envs=None):
    """`world` ranks of the worker, each waited for with a timeout; on a failure or a timeout every
    remaining rank is killed before the assertion.  No retries."""
    assert world <= 4
    port, n = _port(), (envs or GLOBAL_ENVS) // world
    procs, outs = [], []
    for r in range(world):
        out = os.path.join(tmp, f"{mode}_{arg if mode in ('fit', 'one') else 'ck'}_w{world}_r{r}.pt")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "sharded_lr_worker.py"), mode, out, str(n),
                                       arg], env=env))
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


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """Per arm, started on first use: the plain one-rank run and the run over a gloo group of one."""
    cache, tmp = {}, str(tmp_path_factory.mktemp("one"))

    def get(arm):
        if arm not in cache:
            cache[arm] = launch(tmp, 1, "one", arm)[0]
        return cache[arm]
    return get


def assert_same(a, b, what):
    for key in SAME:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (what, key)
    assert a["optimizer_state"] == b["optimizer_state"] and a["step_count"] == b["step_count"], what


def check_rows(res, arm):
    """What every run of an arm must show, on its own optimizer table."""
    from dexterous_rl_manipulation_amd.lr_control import lr_nominal
    o, cfg = res["optimizer"], K.config(arm)
    assert o.shape == (K.ITERS, len(R.COLUMNS)) and res["table"].shape[0] == K.ITERS and res["step_count"] == 4 * K.ITERS
    assert (o[:, COL["updates"]] + o[:, COL["skipped"]]).tolist() == [4.0] * K.ITERS
    assert np.isfinite(o).all() and (o[:, COL["kl_max"]] >= o[:, COL["kl_epoch"]]).all()
    if arm == "stop":  # pass 0 runs on the rollout's own weights (KL 0 <= 1.5e-9) and is applied; pass 1 stops
        assert o[:, COL["stop_pass"]].tolist() == [1.0] * K.ITERS and o[:, COL["updates"]].tolist() == [1.0] * K.ITERS
        assert res["optimizer_state"]["applied"] == K.ITERS and res["optimizer_state"]["skipped"] == 3 * K.ITERS
    scale = 1.0
    for i in range(K.ITERS):  # lr of the first applied pass: the schedule x the scale the iteration began with, clamped
        want = min(max(lr_nominal(cfg, i) * scale, cfg.lr_min), cfg.lr_max)
        assert o[i, COL["updates"]] >= 1.0 and o[i, COL["lr"]] == want, (arm, i)
        scale = o[i, COL["lr_scale"]]
    assert res["optimizer_state"]["scale"] == scale
    if arm == "adapt":
        # the schedule moved: the nominal rate falls every iteration, so no two rows share their lr
        assert len(set(o[:, COL["lr"]].tolist())) == K.ITERS
        # and the adaptation followed the band rule on the row's own kl_epoch: the next scale of
        # every row recomputed on the host (the clamps of [lr_min, lr_max] are far from these rates)
        scale, moved = 1.0, 0
        for i in range(K.ITERS):
            kl, want = o[i, COL["kl_epoch"]], scale
            if kl > cfg.kl_adapt_band * cfg.target_kl:
                want = scale / cfg.kl_adapt_factor
            elif kl < cfg.target_kl / cfg.kl_adapt_band:
                want = scale * cfg.kl_adapt_factor
            assert cfg.lr_min < lr_nominal(cfg, i) * want < cfg.lr_max and o[i, COL["lr_scale"]] == want, i
            moved += want != scale
            scale = want
        print(f"{arm}: kl_epoch {o[:, COL['kl_epoch']].tolist()}, lr_scale {o[:, COL['lr_scale']].tolist()}")
        assert moved >= 1  # the arm exercises the adaptation, not only the recomputation


@pytest.mark.parametrize("arm", ["stop", "adapt"])
@pytest.mark.parametrize("world", [2, 4])
def test_ranks_decide_alike_from_the_global_kl(tmp_path, one_rank, world, arm):
    ranks = launch(str(tmp_path), world, "fit", arm)
    for r, res in enumerate(ranks[1:], 1):
        assert_same(ranks[0], res, f"rank {r}")
    assert all(res["collective"] for res in ranks)
    check_rows(ranks[0], arm)
    got, ref = ranks[0]["optimizer"][0, COL["kl_max"]], one_rank(arm)["plain"]["optimizer"][0, COL["kl_max"]]
    print(f"world {world} {arm}: row 0 kl_max {got!r}, one rank {ref!r}, |diff| {abs(got - ref):.3e}")
    assert abs(got - ref) <= 1e-4 * max(1.0, abs(ref))


@pytest.mark.parametrize("arm", ["stop", "adapt"])
def test_a_group_of_one_rank_is_the_plain_trainer(one_rank, arm):
    res = one_rank(arm)
    assert res["grouped"]["collective"] and not res["plain"]["collective"]
    assert_same(res["plain"], res["grouped"], arm)
    check_rows(res["plain"], arm)


def test_sharded_controlled_run_resumes_bit_for_bit(tmp_path):
    ranks = launch(str(tmp_path), 2, "resume", str(tmp_path))
    for r, res in enumerate(ranks):
        assert_same(res["straight"], res["resumed"], f"rank {r}")
    assert_same(ranks[0]["straight"], ranks[1]["straight"], "ranks")
    assert ranks[0]["saved_opt_state"].tobytes() == ranks[1]["saved_opt_state"].tobytes()  # every file, the same block
    check_rows(ranks[0]["resumed"], "adapt")



def test_cli_resumes_a_sharded_controlled_run(tmp_path):
    """`train --gpus 2 --resume DIR` of a controlled sharded run: the step-size settings and the
    state block come from the rank checkpoints (a resuming command line names no step-size flag),
    the run goes on over the KL exchange, and its optimizer table continues the checkpoint's."""
    from dexterous_rl_manipulation_amd import train, training_run
    ck, out = tmp_path / "ck", tmp_path / "more"
    ck.mkdir()
    ranks = launch(str(tmp_path), 2, "cli_ckpt", str(ck), envs=128)
    assert_same(ranks[0], ranks[1], "ranks")
    assert train.main(["--gpus", "2", "--backend", "gloo"] + K.CLI_ARGS + ["--iterations", "1", "--out", str(out),
                                                                             "--resume", str(ck)]) == 0
    log = training_run.TrainingLog.load(out / "training_log.json")
    assert len(log) == 3 and log.optimizer is not None and len(log.optimizer) == 3
    assert log.optimizer.table[:2].tobytes() == ranks[0]["optimizer"].tobytes()
    assert log.optimizer["updates"][2] + log.optimizer["skipped"][2] == 2.0
    blocks = [training_run.read_checkpoint(out / f"checkpoint.rank{r}.npz")[0]["opt_state"] for r in range(2)]
    assert blocks[0].tobytes() == blocks[1].tobytes() != ranks[0]["opt_state"].tobytes()
