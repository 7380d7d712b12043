"""CPU tests of the robustness analysis (robustness_analysis.py) and of the C ABI of
``dxrl_robustness_summarize``.

1. ``analyze_robustness_results`` / ``print_robustness_report`` against the reference's recording
   (tests/golden/robustness_golden.json): dictionaries equal with ``==``, key order included, and
   the text character for character;
2. ``plot_robustness_results`` writes a PNG with and without combined levels;
3. the ctypes mirror of ``dxrl_robustness_summary_args`` has the C layout (gcc probe), the header
   declares the entry point, ``_SIGS`` holds it, and the call rejects bad arguments before it
   touches a device.
"""
import contextlib
import ctypes as C
import functools
import io
import json
import os
import subprocess

import pytest

import dexterous_rl_manipulation_amd as pkg
from dexterous_rl_manipulation_amd import robustness_analysis as ra

from test_native_abi import HEADER, declared_functions, native  # noqa: F401  (native: fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robustness_golden.json")
FAMILIES = ("observation_noise", "dynamics_noise", "combined_noise")


@functools.lru_cache(None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def from_pairs(rec, suffix=""):
    """A recorded results / analysis dict with its [key, value] pair lists back as dictionaries
    (float keys for the observation and dynamics levels, as the sweep writes them)."""
    out = {"baseline": rec["baseline"]}
    for fam in FAMILIES:
        out[fam + suffix] = {k: v for k, v in rec[fam + suffix]}
    return out


def same_ordered(a, b):
    """``==`` on every leaf and the same key order at every level."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys()), (list(a), list(b))
        for k in a:
            same_ordered(a[k], b[k])
    else:
        assert type(a) is type(b) and a == b, (a, b)


def report_text(analysis):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ra.print_robustness_report(analysis)
    return buf.getvalue()


def cases():
    g = golden()
    return g["hand_written"] + [g["real"]]


# ------------------------------------------------------------------ 1. analysis and report
@pytest.mark.parametrize("i", range(3))
def test_analysis_and_report_match_reference(i):
    rec = cases()[i]
    results = from_pairs(rec["results"])
    want = from_pairs(rec["analysis"], "_degradation")
    assert list(want) == ["baseline"] + [f + "_degradation" for f in FAMILIES]
    got = ra.analyze_robustness_results(results)
    same_ordered(got, want)
    assert report_text(got) == rec["text"]


def test_golden_covers_the_branches():
    zero, pos = golden()["hand_written"]
    a0 = from_pairs(zero["analysis"], "_degradation")
    assert zero["base_rate"] == 0.0
    assert all(r["degradation_percentage"] == 0.0 for f in FAMILIES for r in a0[f + "_degradation"].values())
    assert any(r["degradation"] < 0 for r in a0["dynamics_noise_degradation"].values())
    keys = list(a0["observation_noise_degradation"])
    assert keys != sorted(keys) and a0["combined_noise_degradation"] == {}
    a1 = from_pairs(pos["analysis"], "_degradation")
    assert any(r["degradation_percentage"] < 0 for r in a1["dynamics_noise_degradation"].values())
    real = from_pairs(golden()["real"]["analysis"], "_degradation")
    assert len(real["combined_noise_degradation"]) == 4
    assert len({r["success_rate"] for f in FAMILIES for r in real[f + "_degradation"].values()}) > 1


def test_public_surface():
    from dexterous_rl_manipulation_amd import evaluation as ev
    for name in ra.__all__:
        assert getattr(ev, name) is getattr(ra, name)
    assert pkg.robustness_analysis is ra
    import inspect
    sig = inspect.signature(ra.run_robustness_study)
    assert list(sig.parameters)[:6] == ["policy", "eval_config", "observation_noise_levels", "dynamics_noise_levels",
                                        "num_episodes", "seed"]
    assert sig.parameters["parallel"].default is True and sig.parameters["num_episodes"].default == 20
    assert list(inspect.signature(ra.plot_robustness_results).parameters) == ["results", "analysis", "output_path"]
    assert inspect.signature(ra.plot_robustness_results).parameters["output_path"].default == \
        "logs/robustness_analysis.png"


# ------------------------------------------------------------------ 2. the figure
@pytest.mark.parametrize("i", [0, 2])
def test_plot_writes_a_png(tmp_path, i):
    rec = cases()[i]
    results = from_pairs(rec["results"])
    analysis = ra.analyze_robustness_results(results)
    assert bool(analysis["combined_noise_degradation"]) == (i == 2)
    path = tmp_path / "robustness.png"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ra.plot_robustness_results(results, analysis, str(path))
    assert buf.getvalue() == f"Robustness analysis plot saved to {path}\n"
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 10000


# ------------------------------------------------------------------ 3. the C ABI
def test_struct_layout_matches_c(native, tmp_path):  # noqa: F811
    s, mirror = "dxrl_robustness_summary_args", native.RobustnessSummaryArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));']
    lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f, _ in mirror._fields_]
    lines.append("return 0;}")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got[s]) == C.sizeof(mirror) == 6 * 4 + 15 * 8
    for f, _ in mirror._fields_:
        assert int(got[f"{s}.{f}"]) == getattr(mirror, f).offset, f
    assert len(got) == 1 + len(mirror._fields_)  # every member of the C struct is mirrored (sizes agree)


def test_entry_point_is_declared_and_bound(native):  # noqa: F811
    assert "dxrl_robustness_summarize" in declared_functions()
    res, args = native._SIGS["dxrl_robustness_summarize"]
    assert res is C.c_int and args[1]._type_ is native.RobustnessSummaryArgs and len(args) == 3
    assert hasattr(native.lib(), "dxrl_robustness_summarize")
    assert native.lib().dxrl_abi_version() == native.ABI_VERSION == 1
    src = open(HEADER).read()
    assert "robustness_analysis.py:12-77" in src and "metrics.py:39-103,128-206" in src


def test_argument_checks_run_before_any_device_work(native):  # noqa: F811
    fake = 1 << 20  # never dereferenced: the checks run first
    ptrs = [f for f, t in native.RobustnessSummaryArgs._fields_ if t is C.c_void_p]

    def args(**kw):
        a = native.RobustnessSummaryArgs()
        a.total_episodes, a.max_steps, a.success_threshold, a.num_groups, a.num_members, a.tie_cap = 4, 10, 3, 2, 4, 4
        for f in ptrs:
            setattr(a, f, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rejected(match, **kw):
        with pytest.raises(ValueError, match=match):
            native.call("dxrl_robustness_summarize", 0, C.byref(args(**kw)), None)

    with pytest.raises(ValueError, match="null args"):
        native.call("dxrl_robustness_summarize", 0, None, None)
    rejected("max_steps", max_steps=0)
    rejected("max_steps", max_steps=native.SUMMARY_MAX_STEPS + 1)
    for k in ("total_episodes", "num_groups", "num_members"):
        rejected("must be >= 0", **{k: -1})
    for k in ("ep_length", "ep_success", "ep_contacts", "ep_return", "hist_moments"):
        rejected("episode record", **{k: None})
    rejected("group table", group_offsets=None)
    rejected("group table", group_episodes=None)
    rejected("baseline_group", baseline_group=None)
    for k in ("group_stats", "group_return", "level_table", "tie_count", "status"):
        rejected("null group_stats", **{k: None})
    rejected("tie_list", tie_list=None)
    rejected("tie_list", tie_cap=-1)
