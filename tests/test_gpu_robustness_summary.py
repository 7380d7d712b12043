"""GPU tests of the device robustness summary (``dxrl_robustness_summarize``,
csrc/dxrl_robustness_summary.hip), buffers uploaded directly.

1. rules: on the synthetic records of tests/eval_summary_reference.py, given only as their
   history moments, ``ep_code`` equals the restatement's codes for every row (tie rows coded as
   not unstable) and the tie list equals its tie mask, ascending;
2. groups: ``group_stats`` / ``group_return`` are byte-identical to ``dxrl_eval_summarize`` on the
   same records with their histories, and equal the restatement (integers exact, mean and M2 to
   1e-9);
3. degradation: ``level_table`` equals the reference's four Python-float expressions with ``==``
   (NaN positions equal) for baselines that are absent, the level itself, a later group, empty
   and all failures; an entry outside [-1, G) sets status bit 2 and spoils no other row;
4. status bits, bit-identical launches, E = 0 and G = 0.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dexterous_rl_manipulation_amd import _native as N
from dexterous_rl_manipulation_amd import evaluator as evr

import eval_summary_reference as R
from test_gpu_eval_summary import Guarded
from test_gpu_eval_summary import summarize as eval_summarize

pytestmark = pytest.mark.gpu


def moments_of(d, max_steps):
    """i32 [E][5] S1, S2, first-five, last-five (the restatement's episode pass) and the peak,
    taken as the row maximum."""
    code, mom, tie = R.episode_pass(d["length"], d["success"], d["contacts"], d["hist"], max_steps)
    peak = [int(d["hist"][e, :d["length"][e]].max()) if d["length"][e] else 0 for e in range(len(mom))]
    return code, tie, np.concatenate([mom, np.asarray(peak, np.int32).reshape(-1, 1)], 1).astype(np.int32)


def summarize(d, mom, max_steps, groups, baseline, tie_cap=16, members=None, want_code=True):
    """One dxrl_robustness_summarize on the records ``d`` (no history: ``mom`` only); returns every
    output as NumPy."""
    dev = torch.device("cuda", torch.cuda.current_device())
    E = len(d["length"])
    off, mem = evr.group_table(groups)
    if members is not None:
        mem = np.asarray(members, np.int32)
    G = len(off) - 1
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)  # noqa: E731
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
    ins = [t(pad(d["length"]), np.int32), t(pad(d["success"]), np.uint8), t(pad(d["contacts"]), np.uint8),
           t(pad(d["ret"]), np.float64), t(mom if E else np.zeros((1, 5)), np.int32), t(off, np.int32),
           t(pad(mem), np.int32), t(pad(np.asarray(baseline, np.int32)), np.int32)]
    out = dict(code=Guarded(E, np.int8, (E,), dev), stats=Guarded(128 * G, np.int64, (G, 16), dev),
               ret=Guarded(24 * G, np.float64, (G, 3), dev), level=Guarded(32 * G, np.float64, (G, 4), dev),
               tie_count=Guarded(4, np.int32, (1,), dev), ties=Guarded(4 * tie_cap, np.int32, (tie_cap,), dev),
               status=Guarded(4, np.int32, (1,), dev))
    a = N.RobustnessSummaryArgs()
    a.total_episodes, a.max_steps, a.success_threshold, a.num_groups = E, max_steps, 3, G
    a.num_members, a.tie_cap = len(mem), tie_cap
    (a.ep_length, a.ep_success, a.ep_contacts, a.ep_return, a.hist_moments, a.group_offsets, a.group_episodes,
     a.baseline_group) = (x.data_ptr() for x in ins)
    a.group_stats, a.group_return, a.level_table = out["stats"].ptr, out["ret"].ptr, out["level"].ptr
    a.ep_code = out["code"].ptr if want_code else None
    a.tie_count, a.tie_list, a.status = out["tie_count"].ptr, out["ties"].ptr, out["status"].ptr
    N.call("dxrl_robustness_summarize", dev.index, C.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return {k: v.get() for k, v in out.items()}  # Guarded.get checks the guard zones


# ------------------------------------------------------------------ 1. rules
@pytest.mark.parametrize("max_steps,n_pairs", [(37, 12), (16, 11)])
def test_rules_on_synthetic_records(max_steps, n_pairs, monkeypatch):
    # synthetic_rules takes its searched tie rows at lengths up to 29, which a pitch of 16 cannot
    # hold: search them at lengths the pitch holds (the same search, the same seed)
    search = R.var_tie_rows
    monkeypatch.setattr(R, "var_tie_rows",
                        lambda want=3, seed=2024, max_n=30: search(want, seed, min(max_n, max_steps + 1)))
    d = R.synthetic_rules(max_steps, n_pairs)
    assert d["length"].max() == max_steps
    E = len(d["length"])
    code, tie, mom = moments_of(d, max_steps)
    assert 1 <= tie.sum() <= 8 and set(np.unique(code)) == set(range(-1, 6))
    out = summarize(d, mom, max_steps, [np.arange(E)], [0], tie_cap=16)
    assert out["status"][0] == 0
    assert np.array_equal(out["code"], code)  # every row, the tie rows too
    assert (out["code"][tie] != R.UNSTABLE).all()
    nt = int(out["tie_count"][0])
    assert nt == tie.sum() and out["ties"][:nt].tolist() == np.flatnonzero(tie).tolist()
    stats, _ = R.group_pass(code, tie, d["length"], d["success"], d["contacts"], d["ret"], [np.arange(E)])
    assert np.array_equal(out["stats"], stats) and out["stats"][0, 13] == nt
    # a different garbage peak changes nothing: the word is not read
    other = mom.copy()
    other[:, 4] = 255
    again = summarize(d, other, max_steps, [np.arange(E)], [0], tie_cap=16)
    assert all(out[k].tobytes() == again[k].tobytes() for k in out)


# ------------------------------------------------------------------ 2./3. groups and degradation
E_GROUPS, PITCH, TIE_CAP = 1300, 23, 1300


@pytest.fixture(scope="module")
def case():
    d = R.random_records(E_GROUPS, PITCH)
    rng = np.random.default_rng(11)
    d["ret"][:300] = -1e6 + rng.normal(0.0, 1e-3, 300)  # returns of the form big + small
    code, tie, mom = moments_of(d, PITCH)
    fails = np.flatnonzero(d["success"] == 0)[:40]
    groups = [np.zeros(0, np.int64),                      # 0 empty
              np.array([17]),                             # 1 a single member
              np.arange(200, 457),                        # 2 257 members: one more than the workgroup
              np.arange(100, 1125),                       # 3 1025: one more than four batches of 256
              np.array([5, 5, 9, 5, 1299, 9, 0, 0]),      # 4 repeated members
              np.arange(E_GROUPS)[::-1].copy(),           # 5 all episodes, reversed
              fails,                                      # 6 failures only: rate 0.0
              np.arange(0, 300)]                          # 7 the big + small returns
    stats, gret = R.group_pass(code, tie, d["length"], d["success"], d["contacts"], d["ret"], groups)
    assert stats[6, 1] == 0 and 0 < stats[5, 1] < stats[5, 0] and tie.sum() > 16
    return d, mom, code, tie, groups, stats, gret


#           -1, later group, self, empty baseline, all-failure baseline, earlier, forward, all-failure
BASELINE = [-1, 5, 2, 0, 6, 3, 7, 6]


def expected_levels(stats, baseline):
    """The reference's four floats per level in Python arithmetic (robustness_analysis.py:22-47 on
    metrics.py's rates), NaN where the issue's contract says so."""
    G = len(stats)
    nan = float("nan")
    rate = [int(s[1]) / int(s[0]) if s[0] else nan for s in stats]
    out = []
    for g in range(G):
        n, b = int(stats[g, 0]), baseline[g]
        row = [rate[g], int(stats[g, 2]) / n if n else nan, nan, nan]
        if 0 <= b < G and n and stats[b, 0]:
            baseline_success = rate[b]
            degradation = baseline_success - rate[g]
            row[2] = degradation
            row[3] = (degradation / baseline_success * 100) if baseline_success > 0 else 0.0
        out.append(row)
    return out


def same_floats(got, want):
    for g, (a, b) in enumerate(zip(got.tolist(), want)):
        for k in range(4):
            assert (math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], (g, k, a, b)


def test_groups_are_bit_identical_to_the_history_summary(case):
    d, mom, code, tie, groups, stats, gret = case
    out = summarize(d, mom, PITCH, groups, BASELINE, tie_cap=TIE_CAP)
    ref, _ = eval_summarize(d, PITCH, groups, tie_cap=TIE_CAP)
    assert out["status"][0] == 0 and ref["status"][0] == 0
    assert np.array_equal(out["stats"].view(np.uint8), ref["stats"].view(np.uint8))
    assert np.array_equal(out["ret"].view(np.uint8), ref["ret"].view(np.uint8))
    assert np.array_equal(out["code"], ref["code"]) and np.array_equal(out["code"], code)
    assert out["tie_count"][0] == ref["tie_count"][0] == tie.sum()
    assert np.array_equal(out["ties"][:tie.sum()], np.flatnonzero(tie))
    assert np.array_equal(out["stats"], stats)
    assert np.array_equal(out["ret"][0], [0.0, 0.0, 0.0])
    for g, idx in enumerate(groups):
        if not len(idx):
            continue
        n, mean, m2 = out["ret"][g]
        assert n == len(idx)
        assert mean == pytest.approx(gret[g, 1], rel=1e-9)
        assert m2 == pytest.approx(gret[g, 2], rel=1e-9, abs=0.0 if len(idx) > 1 else 1e-300)


def test_level_table_equals_the_python_floats(case):
    d, mom, code, tie, groups, stats, gret = case
    out = summarize(d, mom, PITCH, groups, BASELINE, tie_cap=TIE_CAP, want_code=False)
    assert out["status"][0] == 0
    want = expected_levels(stats, BASELINE)
    same_floats(out["level"], want)
    lv = out["level"]
    assert np.isnan(lv[0]).all() and np.isnan(lv[3, 2:]).all() and not np.isnan(lv[3, :2]).any()
    assert lv[2, 2] == 0.0 and lv[2, 3] == 0.0                        # its own baseline
    assert lv[4, 3] == 0.0 and lv[4, 2] < 0 and lv[7, 3] == 0.0      # baseline rate 0.0: percentage exactly 0.0
    assert lv[6, 2] > 0 and lv[6, 3] == 100.0                         # all failures against a forward baseline
    assert not np.isnan(lv[1]).any() and not np.isnan(lv[5]).any()


@pytest.mark.parametrize("bad", [8, -2])
def test_baseline_out_of_range_sets_status_bit_2(case, bad):
    d, mom, code, tie, groups, stats, gret = case
    base = list(BASELINE)
    base[3] = bad  # G itself, or below -1
    out = summarize(d, mom, PITCH, groups, base, tie_cap=TIE_CAP)
    assert out["status"][0] == 4
    same_floats(out["level"], expected_levels(stats, base))
    assert np.isnan(out["level"][3, 2:]).all() and not np.isnan(out["level"][3, :2]).any()
    assert np.array_equal(out["stats"], stats)


# ------------------------------------------------------------------ 4. status, determinism, empty
def test_status_bits(case):
    d, mom, code, tie, groups, stats, gret = case
    out = summarize(d, mom, PITCH, groups, BASELINE, tie_cap=3)
    assert out["status"][0] == 2 and out["tie_count"][0] == tie.sum() > 3
    assert out["ties"].tolist() == np.flatnonzero(tie)[:3].tolist()
    off, mem = evr.group_table(groups)
    bad = mem.copy()
    bad[off[2] + 5] = E_GROUPS   # one member of group 2 past the records
    bad[off[3] + 1] = -3         # one of group 3 before them
    out = summarize(d, mom, PITCH, groups, BASELINE, tie_cap=TIE_CAP, members=bad)
    assert out["status"][0] == 1
    good = [np.asarray(g) for g in groups]
    good[2] = np.delete(good[2], 5)
    good[3] = np.delete(good[3], 1)
    want, _ = R.group_pass(code, tie, d["length"], d["success"], d["contacts"], d["ret"], good)
    assert np.array_equal(out["stats"], want)  # the bad members are skipped, everything else counted
    same_floats(out["level"], expected_levels(want, BASELINE))


def test_two_launches_are_bit_identical(case):
    d, mom, code, tie, groups, stats, gret = case
    a = summarize(d, mom, PITCH, groups, BASELINE, tie_cap=TIE_CAP)
    b = summarize(d, mom, PITCH, groups, BASELINE, tie_cap=TIE_CAP)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.isfinite(a["ret"]).all()


def test_no_episodes_and_no_groups(case):
    d, mom = case[0], case[1]
    none = {k: v[:0] for k, v in d.items()}
    out = summarize(none, mom[:0], PITCH, [np.zeros(0, np.int64), np.zeros(0, np.int64)], [-1, 0], tie_cap=4)
    assert out["status"][0] == 0 and out["tie_count"][0] == 0
    assert not out["stats"].any() and np.isnan(out["level"]).all()
    out = summarize(d, mom, PITCH, [], [], tie_cap=TIE_CAP)
    assert out["status"][0] == 0 and out["tie_count"][0] == case[3].sum()
    assert np.array_equal(out["code"], case[2]) and out["stats"].shape == (0, 16)
