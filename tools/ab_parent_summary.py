"""Verdict of an alternating parent (P) / HEAD (H) run: per figure the two medians, the parent's own
spread over its rounds (max - min: what the box cannot resolve) and whether HEAD's median is
slower than the parent's by more than that spread.

    python tools/ab_parent_summary.py LOG

LOG lines are "<P|H> r<round> <tool output>" for tools/rollout_time.py (with " envs=N" appended),
tools/eval_bench.py, tools/eval_mlp_bench.py and tools/step_bench.py.  All figures are ms."""
import json
import re
import statistics
import sys
from collections import defaultdict

vals = defaultdict(lambda: {"P": [], "H": []})
for line in open(sys.argv[1]):
    m = re.match(r"([PH]) r\d+ (.*)", line.rstrip())
    if not m:
        continue
    v, rest = m.groups()
    if rest.startswith("{"):
        d = json.loads(rest)
        key = f"eval_mlp {d['policy']}" if "policy" in d else "eval_ls " + d["workload"].split()[1]
        vals[key][v].append(d["kernel_ms"])
    elif rest.startswith("variant="):
        vals["k_step 4M envs"][v].append(float(re.search(r"median ms=([\d.]+)", rest).group(1)))
    else:
        cur, envs = rest.split()[0], re.search(r"envs=(\d+)", rest).group(1)
        for name, ms in re.findall(r"(\S+)=([\d.]+)", rest.split(" envs=")[0]):
            vals[f"rollout {name} {cur} {envs}"][v].append(float(ms))

print(f"{'figure (ms)':34s} {'P median':>9s} {'H median':>9s} {'H - P':>8s} {'P spread':>9s} {'H spread':>9s}  verdict")
bad = 0
for key, d in vals.items():
    p, h = d["P"], d["H"]
    mp, mh, sp, sh = statistics.median(p), statistics.median(h), max(p) - min(p), max(h) - min(h)
    ok = mh - mp <= sp
    bad += not ok
    print(f"{key:34s} {mp:9.4f} {mh:9.4f} {mh - mp:+8.4f} {sp:9.4f} {sh:9.4f}  {'ok' if ok else 'SLOWER'}"
          f"  ({len(p)} / {len(h)} rounds)")
print(f"figures: {len(vals)}; HEAD slower than the parent by more than the parent's spread: {bad}")
sys.exit(1 if bad else 0)
