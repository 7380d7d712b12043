"""GPU, multi-rank: fit(merge_ranks=True) on sharded trainers (processes on cuda:0 over gloo, as
tests/test_gpu_dist.py runs them; at most 4 ranks at once), the sharded checkpoint round trip, and
`train --gpus 2`.  256 global envs, horizon 32, episodes capped at 40 steps, 3 iterations.

Every rank finishes every row from the same gathered records, so tables, headers, best parameters
and per-rank records must be byte-equal across ranks.  Against the definitions
(pg_log_reference.row_values on the ranks' concatenated tapes) the bounds are those of
tests/test_gpu_pg_log_world.py: integer-derived columns exact, f64 sums within k 2^-52 sum|x| /
count, variances within 1e-9 relative.  Against the world-1 run on the same 256 envs only the first
row is comparable (the first rollout's tapes are bit-identical, tests/test_gpu_dist.py; afterwards
the parameters drift by f32 reduction order): its tape-derived integer columns are exact, its f64
sums are within the same bound, the advantage statistics within 1e-9 max(1, |ref|) and the loss
columns and grad_norm within 1e-4 max(1, |ref|) -- the bounds test_gpu_dist.py holds the global
moments and the all-reduced gradient to."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import pg_log_reference as L
import pg_log_world_reference as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GLOBAL_ENVS, T, ITERS = 256, 32, 3
WAIT_S = 240


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(tmp, world, mode, arg):
    """Start `world` ranks of the worker and wait for each with a timeout; on any failure or
    timeout every remaining rank is killed before the assertion, so none stays behind with the
    GPU open.  No retries."""
    assert world <= 4
    port, n = _port(), GLOBAL_ENVS // world
    procs, outs = [], []
    for r in range(world):
        out = os.path.join(tmp, f"{mode}_{arg if mode == 'fit' else 'ck'}_w{world}_r{r}.pt")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "sharded_fit_worker.py"), mode, out, str(n),
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
    """The world-1 fit(merge_ranks=True) runs on the 256 envs, one per config, started on first use."""
    cache, tmp = {}, str(tmp_path_factory.mktemp("one"))

    def get(config):
        if config not in cache:
            cache[config] = launch(tmp, 1, "fit", config)[0]
        return cache[config]
    return get


def row_dict(table, r):
    return {name: table[r, k] for k, name in enumerate(L.COLUMNS)}


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_fit_rows_are_identical_and_global(tmp_path, one_rank, world):
    ranks = launch(str(tmp_path), world, "fit", "variable")
    first, n = ranks[0], GLOBAL_ENVS // world
    assert first["table"].shape == (ITERS, L.COLS) and first["ranks"].shape == (ITERS, world, W.RANK_DOUBLES)
    for r, res in enumerate(ranks[1:], 1):
        for key in ("table", "header", "best_params", "ranks"):
            assert res[key].tobytes() == first[key].tobytes(), (r, key)
    table = first["table"]
    episode_means = [L.IDX[k] for k in ("mean_return", "mean_length", "success_rate")]
    for r in range(ITERS):  # every row finite (a row without a finished episode: all but the episode means)
        cols = [k for k in range(L.IS_BEST) if table[r, L.IDX["episodes"]] > 0 or k not in episode_means]
        assert np.isfinite(table[r, cols]).all(), r
    assert table[:, L.IDX["iteration"]].tolist() == [0.0, 1.0, 2.0]
    assert table[:, L.IDX["env_steps"]].tolist() == [float((k + 1) * GLOBAL_ENVS * T) for k in range(ITERS)]
    assert first["env_steps"] == ITERS * GLOBAL_ENVS * T
    # keep-best (mean_return, min_episodes 1) and convergence (mean_return, window 2), restated on the row's values
    score = table[:, L.IDX["mean_return"]].tolist()
    want_rows, want_header, _ = L.series_rules(score, table[:, L.IDX["episodes"]].tolist(), 1, [0.0] * ITERS, 1, 1e300)
    assert table[:, L.IS_BEST].tolist() == [float(r in want_rows) for r in range(ITERS)] and want_rows
    head = first["header_dict"]
    assert (head["rows_written"], head["best_row"], head["best_score"]) == (ITERS, want_rows[-1], score[want_rows[-1]])
    windows = [r for r in range(1, ITERS) if not (math.isnan(score[r - 1]) or math.isnan(score[r]))]
    assert head["converged_row"] == (windows[0] if windows else -1)
    # the records carry each rank's own counts
    assert np.all(first["ranks"][:, :, W.R["samples"]] == n * T)
    assert np.array_equal(first["ranks"][:, :, W.R["episodes"]].sum(1), table[:, L.IDX["episodes"]])

    # the last row against the definitions on the ranks' concatenated last-iteration tapes
    shards = [res["tape"] for res in ranks]
    c = W.concatenated(shards)
    stats, gnorm2 = shards[0]["stats"], shards[0]["gnorm2"]
    assert all(np.array_equal(s["stats"][:5], stats[:5]) and s["gnorm2"] == gnorm2 for s in shards)
    ref = L.row_values(c["n"], T, ITERS - 1, ITERS * GLOBAL_ENVS * T, c["ep_count"], c["ep_sum_return"],
                       c["ep_sum_length"], c["ep_successes"], c["rew"], c["ret"], c["done"], c["values"], stats,
                       c["loss_partial"], c["loss_rows"], gnorm2)
    assert ref["episodes"] > 0
    W.assert_row_within_bounds(row_dict(table, ITERS - 1), ref, c["ep_sum_return"], c["rew"], c["ret"], c["values"],
                               c["loss_partial"], c["loss_rows"], what=f"world {world} last row")

    # row 0 against the world-1 run on the same envs
    one = one_rank("variable")
    assert one["ranks"].shape == (ITERS, 1, W.RANK_DOUBLES)
    got, want, t0 = row_dict(table, 0), row_dict(one["table"], 0), one["tape0"]
    for name in ("iteration", "env_steps", "episodes", "mean_length", "success_rate", "done_fraction"):
        assert got[name] == want[name], name
    M = GLOBAL_ENVS * T
    for name, terms, count in (("mean_return", t0["ep_sum_return"], want["episodes"]), ("mean_step_reward", t0["rew"], M),
                               ("value_mean", t0["values"], M), ("target_mean", t0["ret"], M)):
        if count == 0:  # no episode finished in the first rollout: NaN on both sides
            assert math.isnan(got[name]) and math.isnan(want[name]), name
            continue
        bound = W.sum_bound(terms) / count
        print("row 0", name, got[name], want[name], abs(got[name] - want[name]), bound)
        assert abs(got[name] - want[name]) <= bound, name
    for name in ("adv_mean", "adv_std"):
        assert abs(got[name] - want[name]) <= 1e-9 * max(1.0, abs(want[name])), name
    for name in W.LOSS + ("grad_norm",):
        print("row 0", name, got[name], want[name])
        assert abs(got[name] - want[name]) <= 1e-4 * max(1.0, abs(want[name])), name


def test_sharded_run_validates_and_resumes_bit_for_bit(tmp_path):
    ranks = launch(str(tmp_path), 2, "resume", str(tmp_path))
    for r, res in enumerate(ranks):
        s, v = res["straight"], res["resumed"]
        assert s["table"].shape == (4, L.COLS) and s["val_table"].shape[0] == 2
        assert s["val_table"][:, 0].tolist() == [1.0, 3.0]  # validated after the 2nd and the 4th iteration
        for key in ("params", "m1", "m2", "table", "header", "best_params", "ranks", "val_table", "val_header",
                    "val_best_params", "val_objects"):
            assert v[key].tobytes() == s[key].tobytes(), (r, key)
        assert res["sched"][0] == res["sched"][1]
        assert "world_size" in res["refused"]
    a, b = ranks[0]["straight"], ranks[1]["straight"]
    for key in ("table", "header", "best_params", "ranks", "val_table", "val_header", "val_best_params", "val_objects",
                "params"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert (tmp_path / "checkpoint.rank0.npz").exists() and (tmp_path / "checkpoint.rank1.npz").exists()


def test_cli_trains_on_two_ranks_and_resumes(tmp_path, capfd):
    from dexterous_rl_manipulation_amd import train, training_run
    out = tmp_path / "run"
    common = ["--gpus", "2", "--backend", "gloo", "--envs", "128", "--horizon", "16", "--max-steps", "12"]
    assert train.main(common + ["--iterations", "3", "--out", str(out)]) == 0
    log = training_run.TrainingLog.load(out / "training_log.json")
    assert len(log) == 3 and log.ranks.shape == (3, 2, W.RANK_DOUBLES)
    assert log["env_steps"].tolist() == [2048.0, 4096.0, 6144.0]
    assert np.all(log.rank_column("samples") == 64 * 16)
    metas = []
    for r in range(2):
        arrays, meta = training_run.read_checkpoint(out / f"checkpoint.rank{r}.npz")
        assert (meta["world"], meta["rank"], meta["env"]["global_env_offset"]) == (2, r, 64 * r)
        assert meta["log"]["rows"] == 3 and arrays["log_ranks"].shape == (3, 2, W.RANK_DOUBLES)
        metas.append(arrays)
    assert metas[0]["log_table"].tobytes() == metas[1]["log_table"].tobytes() == log.table.tobytes()
    assert not (out / "checkpoint.npz").exists() and "iterations" in capfd.readouterr().out
    out2 = tmp_path / "more"
    assert train.main(common + ["--iterations", "1", "--out", str(out2), "--resume", str(out)]) == 0
    log2 = training_run.TrainingLog.load(out2 / "training_log.json")
    assert log2["iteration"].tolist() == [0.0, 1.0, 2.0, 3.0] and log2.table[:3].tobytes() == log.table.tobytes()
    assert log2.ranks.shape == (4, 2, W.RANK_DOUBLES) and math.isfinite(log2["grad_norm"][-1])
    assert (out2 / "checkpoint.rank0.npz").exists() and (out2 / "checkpoint.rank1.npz").exists()
    with pytest.raises(SystemExit):
        train.main(["--gpus", "2", "--backend", "gloo", "--envs", "129", "--iterations", "1", "--out", str(out2)])
