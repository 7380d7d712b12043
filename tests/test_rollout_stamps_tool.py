"""CPU: tools/rollout_stamps.py's parsing of the rollout's per-wave stamp lines (the layout the
library prints under diag 128: env / aux means, then one line per wave)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOG = """/opt/amdgpu/share/libdrm/amdgpu.ids: No such file or directory
easy
rollout_ws env cycles/step: s0=262 s1=801 s2=1052 s3=1144 s4=503 s5=2671 s6=135
  wave 0: s0=262 s1=800 s2=1052 s3=1073 s4=573 s5=2668 s6=140
  wave 1: s0=262 s1=802 s2=1051 s3=1079 s4=566 s5=2676 s6=132
  wave 2: s0=262 s1=802 s2=1051 s3=1073 s4=572 s5=2673 s6=134
  wave 3: s0=262 s1=799 s2=1052 s3=1350 s4=302 s5=2669 s6=133
rollout_ws aux cycles/step: s0=306 s1=952 s2=1067 s3=1276 s4=161 s5=2361 s6=445
  wave 4: s0=306 s1=951 s2=1067 s3=1214 s4=222 s5=2358 s6=449
  wave 5: s0=305 s1=953 s2=1066 s3=1272 s4=164 s5=2367 s6=440
  wave 6: s0=306 s1=953 s2=1066 s3=1269 s4=166 s5=2360 s6=448
  wave 7: s0=305 s1=951 s2=1067 s3=1348 s4=93 s5=2359 s6=443
variable noise
rollout_ws env cycles/step: s0=1099 s1=1154 s2=1063 s3=1138 s4=502 s5=2241 s6=441
  wave 0: s0=1099 s1=1156 s2=1062 s3=1070 s4=567 s5=2254 s6=429
  wave 7: s0=1439 s1=1002 s2=1062 s3=1347 s4=110 s5=2348 s6=329
"""


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("rollout_stamps", os.path.join(ROOT, "tools", "rollout_stamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # imports neither torch nor the package
    return mod


def test_parse_keeps_one_record_per_wave_and_config(tool):
    got = tool.parse_stamps(LOG)
    assert list(got) == ["easy", "variable noise"]
    assert sorted(got["easy"]) == list(range(8))
    assert got["easy"][3] == [262, 799, 1052, 1350, 302, 2669, 133]
    assert got["easy"][7][3] == 1348
    assert sorted(got["variable noise"]) == [0, 7]
    assert got["variable noise"][7] == [1439, 1002, 1062, 1347, 110, 2348, 329]


def test_table_names_the_longest_wave_of_each_segment(tool):
    rows = tool.table(tool.parse_stamps(LOG)["easy"]).splitlines()
    assert rows[0].split()[:9] == ["segment"] + [f"w{k}" for k in range(8)]
    head = rows[4].split()  # s3 head phase: wave 3 at 1350
    assert head[:3] == ["s3", "head", "phase"] and head[-2:] == ["1350", "3"]
    p4 = rows[6].split()  # s5 P4: wave 1 at 2676
    assert p4[-2:] == ["2676", "1"]
    sums = rows[-1].split()
    assert sums[0] == "sum" and int(sums[1]) == 262 + 800 + 1052 + 1073 + 573 + 2668 + 140
    assert "easy" in tool.report(LOG) and "variable noise" in tool.report(LOG)


def test_parse_rejects_a_record_with_missing_segments(tool):
    with pytest.raises(ValueError):
        tool.parse_stamps("easy\n  wave 0: s0=1 s2=3\n")
    assert tool.parse_stamps("no stamps here\n") == {}
