"""GPU: k_wgrad_l1's chunk loop (64 x 128 wave tiles, fragments double-buffered in registers,
the recompute's tanh between the contraction's MFMAs) against k_wgrad_glds, which keeps the
32 x 256 wave tiles and the plain loop: the whole gradient vector bit for bit, no tolerance.  A
misplaced output tile, a swapped fragment or a stale prefetched fragment shows on dW2's
256 x 256 block.  The sizes walk the loop's edges: chunk counts per workgroup below, at and
above the ring's look-ahead (3 chunks) with both parities of the H1 double buffer, and ragged
divisions where neighbouring workgroups get k and k + 1 chunks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 32  # samples per chunk (kLK)


@pytest.fixture(scope="module")
def pkg():
    import dexterous_rl_manipulation_amd as d
    from dexterous_rl_manipulation_amd import envs, trainer  # noqa: F401
    return d


def make(pkg, n, T, **kw):
    env = pkg.envs.VecEnv(n, curriculum_config=pkg.CurriculumConfig.variable(), reward_type="dense", seed=3)
    cfg = pkg.trainer.TrainerConfig(horizon=T, seed=1, ent_coef=0.01, **kw)
    tr = pkg.trainer.PGTrainer(env, cfg)
    env.reset(write_obs=False)
    return tr


def per_network_grads(pkg, n, T, splits, h1_recompute):
    tr = make(pkg, n, T, fused=True, h1_recompute=h1_recompute, pair_learner=False)
    assert not tr.paired
    tr.splits = splits  # before the first pass: the partial slabs are sized from it on first use
    tr.rollout()
    for name in [x for x in tr.phases() if x not in ("rollout", "optimizer_step")]:
        getattr(tr, name)()
    torch.cuda.synchronize()
    return tr.grads.clone()


# rows = 32 * chunks; one workgroup unless splits says otherwise
@pytest.mark.parametrize("chunks,splits", [
    (1, 1), (2, 1), (3, 1), (4, 1), (5, 1),  # below, at and above the look-ahead; both H1 parities
    (9, 1),
    (33, 4),   # ragged: 9, 8, 8, 8 chunks
    (7, 2),    # ragged: 4 and 3 chunks, either side of the look-ahead
    (5, 4),    # ragged: 2, 1, 1, 1
])
def test_chunk_loop_equals_copy_path(pkg, chunks, splits):
    """h1_recompute True (k_wgrad_l1) == False (k_wgrad_glds on the H1 copy) at the same split
    count, per-network path."""
    got = per_network_grads(pkg, chunks, CHUNK, splits, True)
    ref = per_network_grads(pkg, chunks, CHUNK, splits, False)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("chunks", [17, 40])  # 17 splits: one chunk each; 2 or 3 chunks each
def test_paired_chunk_loop_equals_two_passes(pkg, chunks):
    """The paired launch (both networks' dW2 in one k_wgrad_l1 grid, the second network's
    workgroups offset by nb0) == two per-network passes at the same split count, at the smallest
    split count the trainer pairs at."""
    outs = []
    for paired in (True, False):
        tr = make(pkg, chunks, CHUNK, pair_splits=17)
        assert tr.paired and tr.pair_splits == 17
        if not paired:
            tr.paired = False
            tr.splits = tr.pair_splits
            tr.kpartial = torch.zeros(tr.splits + 16, 256, 288, device=tr.dev)
        tr.rollout()
        tr.critic_values()
        tr.advantages()
        tr.train_passes()
        torch.cuda.synchronize()
        outs.append((tr.grads.clone(), tr.fused_loss.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
