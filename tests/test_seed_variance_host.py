"""CPU tests of the seed-variance driver and of the host half of the device episode summary:

* the NumPy restatement of ``dxrl_eval_summarize`` (tests/eval_summary_reference.py) plus the
  host tie fix-up equals metrics.classify_columns / aggregate_columns, integers exactly;
* fed the reference's per-seed results, ``compute_variance_statistics`` / ``validate_variance``,
  the printed report and the saved JSON equal tests/golden/seed_variance_golden.json;
* argument checks and the ``SeedVarianceConfig`` mapping.
"""
import contextlib
import functools
import io
import json
import os

import numpy as np
import pytest

from dexterous_rl_manipulation_amd import evaluation as ev
from dexterous_rl_manipulation_amd import evaluator as evr
from dexterous_rl_manipulation_amd import metrics as M
from dexterous_rl_manipulation_amd import seed_variance as sv
from dexterous_rl_manipulation_amd.experiments import CurriculumConfig, ExperimentConfig, SeedVarianceConfig

import eval_summary_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_variance_golden.json")


@functools.lru_cache(None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def host_codes(d, max_steps):
    mom = M.HistoryMoments.from_padded(d["hist"], d["length"])
    return M.classify_columns(d["success"], d["length"], d["contacts"], d["contacts"], mom, max_steps, 3), mom


def settled(d, max_steps, groups):
    """Restatement of both passes, then the host fix-up of the tie rows."""
    code, mom, tie = R.episode_pass(d["length"], d["success"], d["contacts"], d["hist"], max_steps)
    stats, gret = R.group_pass(code, tie, d["length"], d["success"], d["contacts"], d["ret"], groups)
    off, mem = evr.group_table(groups)
    rows = np.flatnonzero(tie)
    unstable = evr.settle_ties(stats, off, mem, rows, code[rows], d["hist"][rows], d["length"][rows])
    final = code.copy()
    final[rows[unstable]] = R.UNSTABLE
    return code, final, mom, tie, stats, gret


RECORD_SETS = [("random", 40, None), ("rules", 40, 11), ("rules", 40, 39), ("rules", 37, 11), ("rules", 37, 36)]


@pytest.mark.parametrize("kind,max_steps,n_pairs", RECORD_SETS)
def test_restatement_equals_metrics(kind, max_steps, n_pairs):
    d = R.random_records(2000, max_steps) if kind == "random" else R.synthetic_rules(max_steps, n_pairs)
    E = len(d["length"])
    rng = np.random.default_rng(3)
    groups = [np.arange(E), np.arange(0, E, 3), rng.choice(E, 65, replace=False), np.zeros(0, np.int64)]
    code, final, mom, tie, stats, gret = settled(d, max_steps, groups)
    want, hm = host_codes(d, max_steps)
    assert np.array_equal(final, want)
    assert np.array_equal(code[~tie], want[~tie])
    assert np.array_equal(mom, np.stack([hm.s1, hm.s2, hm.first5, hm.last5], 1))
    if kind == "rules":
        assert 1 <= tie.sum() <= 8 and (final != code).any()  # the fix-up moves at least one row
    for g, idx in enumerate(groups):
        agg = M.aggregate_columns(d["success"][idx].astype(bool), d["length"][idx], d["contacts"][idx], want[idx])
        got = M.aggregate_sums(stats[g], gret[g])
        if not len(idx):
            assert got == {} and agg == {}
            continue
        for k, v in agg.items():
            if k == "std_episode_length":
                assert got[k] == pytest.approx(v, rel=1e-12)
            else:
                assert got[k] == v, k
        assert got["mean_reward"] == pytest.approx(np.mean(d["ret"][idx]), rel=1e-12)
        assert got["std_reward"] == pytest.approx(np.std(d["ret"][idx]), rel=1e-12)


def test_slippage_expression_is_not_the_integer_rule():
    """The f64 rule (L / 5.0) - (F / 5.0) < -1.0 differs from L - F < -5 on some of the 676 pairs,
    which is why the kernel evaluates the f64 expression."""
    F, L = np.meshgrid(np.arange(26), np.arange(26), indexing="ij")
    f64 = (L.astype(np.float64) / 5.0) - (F.astype(np.float64) / 5.0) < -1.0
    assert (f64 != (L - F < -5)).any()


def _results_by_seed(case):
    return {int(s): r for s, r in case["saved"]["variance_analysis"]["individual_results"].items()}


@pytest.mark.parametrize("i", range(3))
def test_statistics_report_and_json_match_reference(i, tmp_path, monkeypatch):
    g = golden()
    case = g["cases"][i]
    results = _results_by_seed(case)
    an = sv.SeedVarianceAnalyzer(None, None)
    analysis = an.compute_variance_statistics(results)
    want = case["result"]["variance_analysis"]
    assert analysis["seeds"] == want["seeds"] == g["seeds"] and analysis["num_seeds"] == want["num_seeds"]
    assert analysis["variance_stats"] == want["variance_stats"]
    # the reference's quirk: these two keys are looked up where they do not exist
    for key in ("overall_success_rate", "mean_reward"):
        assert analysis["variance_stats"][key]["values"] == [0.0] * len(g["seeds"])
    validation = an.validate_variance(analysis["variance_stats"], g["max_cv_threshold"])
    assert validation == case["result"]["validation"]
    ext = an.compute_variance_statistics(results, extended=True)
    assert ext["variance_stats"] == want["variance_stats"]
    assert ext["variance_stats_extended"]["mean_reward"]["values"] == [
        results[s]["overall_stats"]["mean_reward"] for s in g["seeds"]]

    # the whole driver with the evaluations replaced by the reference's per-seed results
    def fake(self, seeds, num_episodes_per_object=5):
        for s in seeds:
            print(f"  Evaluating with seed {s}...")
        return {s: results[s] for s in seeds}

    monkeypatch.setattr(sv.SeedVarianceAnalyzer, "evaluate_multiple_seeds", fake)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = sv.analyze_seed_variance(None, None, seeds=list(g["seeds"]), num_episodes_per_object=g["K"],
                                       max_episode_steps=g["max_steps"], output_dir=str(tmp_path),
                                       max_cv_threshold=g["max_cv_threshold"])
    assert buf.getvalue().replace(str(tmp_path), "<output_dir>") == case["report"]
    assert out["validation"] == case["result"]["validation"]
    with open(tmp_path / "seed_variance_analysis.json") as f:
        assert json.load(f) == case["saved"]
    assert (tmp_path / "seed_variance.png").stat().st_size > 0


def test_fewer_than_three_seeds():
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="At least 3 seeds"):
        sv.analyze_seed_variance(None, None, seeds=[1, 2])


def test_device_summary_argument_checks(monkeypatch):
    """Refused before any device call: the native layer is made unreachable."""
    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(evr.N, "call", no_device)
    monkeypatch.setattr(evr.N, "require_gpu", no_device)
    h = ev.HeldOutObjectSet(CurriculumConfig.medium(), num_heldout_objects=2, seed=1)

    class Space:
        low, high, shape = -np.ones(15, np.float32), np.ones(15, np.float32), (15,)
        np_random = np.random.default_rng(0)

    import dexterous_rl_manipulation_amd as pkg
    pol = pkg.policies.HeuristicPolicy(Space())
    with pytest.raises(ValueError, match="return_episodes=False"):
        ev.Evaluator(pol, h).evaluate_heldout_set(1, seed=0, device_summary=True)
    with pytest.raises(ValueError, match="failure_logger"):
        ev.Evaluator(pol, h, failure_logger=object()).evaluate_heldout_set(1, seed=0, return_episodes=False,
                                                                           device_summary=True)

    class HostPolicy:
        def select_action(self, obs):
            return np.zeros(15, np.float32)

    with pytest.raises(ValueError, match="compiles"):
        ev.Evaluator(HostPolicy(), h).evaluate_heldout_set(1, seed=0, return_episodes=False, device_summary=True)


@pytest.mark.parametrize("wrap", [False, True])
def test_run_seed_variance_maps_every_field(wrap, monkeypatch):
    seen = {}

    def fake(policy, heldout_set, **kw):
        seen.update(kw, policy=policy, heldout_set=heldout_set)
        return "done"

    monkeypatch.setattr(sv, "analyze_seed_variance", fake)
    c = SeedVarianceConfig(seeds=[5, 6, 7, 8], num_episodes_per_object=9, max_episode_steps=33, max_cv_threshold=0.35,
                           reward_type="sparse")
    cfg = ExperimentConfig(seed_variance=c) if wrap else c
    assert sv.run_seed_variance(cfg, "pol", "set", output_dir="somewhere", parallel=True) == "done"
    assert seen == dict(policy="pol", heldout_set="set", seeds=[5, 6, 7, 8], num_episodes_per_object=9,
                        reward_type="sparse", max_episode_steps=33, output_dir="somewhere", max_cv_threshold=0.35,
                        parallel=True)
    fields = {f for f in SeedVarianceConfig.__dataclass_fields__}
    assert fields == {"seeds", "num_episodes_per_object", "max_episode_steps", "max_cv_threshold", "reward_type"}
