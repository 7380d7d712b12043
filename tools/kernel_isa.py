"""Code-generation check for a refactor: per-kernel resources and instruction streams of two trees.

    python tools/kernel_isa.py emit OUTDIR [REV]      # gfx950 assembly + resource remarks of csrc (of commit REV)
    python tools/kernel_isa.py compare DIR_A DIR_B [OLD=NEW ..]   # table A vs B per kernel, "same ISA" yes / no

emit compiles the env / rollout / eval translation units with build.py's FLAGS plus
--cuda-device-only -S -Rpass-analysis=kernel-resource-usage (no GPU needed).  compare matches
kernels by name across all files (a kernel may move between files) and calls two instruction
streams the same when they are equal after dropping comments, debug directives and the kernel's
own name, and renumbering labels in order of appearance.  OLD=NEW: a kernel of A whose demangled
name starts with OLD is compared with the kernel of B whose name starts with NEW (a kernel that
became a template instantiation: "dxrl::k_gae(=void dxrl::k_gae<false>(").  A template's code sits in
a section of its own, so section directives are dropped too."""
import os
import re
import subprocess
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dexterous-rl-manipulation_amd"))
import build as B  # noqa: E402

UNITS = ["dxrl_env", "dxrl_rollout", "dxrl_pg", "dxrl_pg_gae", "dxrl_pg_rollout16", "dxrl_pg_rollout8", "dxrl_eval", "dxrl_eval_mlp"]
FIELDS = ["VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]


def emit(outdir, rev=None):
    os.makedirs(outdir, exist_ok=True)
    csrc = B.CSRC
    if rev:  # the sources of an older commit, mirrored at the real depth ("../../include/dxrl.h")
        src_root = os.path.join(outdir, "_src")
        csrc = os.path.join(src_root, "pkg", "csrc")
        for sub, dst in (("dexterous-rl-manipulation_amd/csrc", csrc), ("include", os.path.join(src_root, "include"))):
            os.makedirs(dst, exist_ok=True)
            tar = subprocess.run(["git", "archive", rev, sub], cwd=ROOT, check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "--strip-components", str(sub.count("/") + 1), "-C", dst], input=tar, check=True)
    flags = [f for f in B.FLAGS if f != "-shared"] + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]

    def one(u):
        src = os.path.join(csrc, u + ".hip")
        if not os.path.exists(src):
            return
        r = subprocess.run([B.HIPCC, *flags, "-o", os.path.join(outdir, u + ".s"), src], cwd=csrc, check=True,
                           capture_output=True, text=True)
        open(os.path.join(outdir, u + ".remarks"), "w").write(r.stderr)

    with ThreadPoolExecutor(min(len(UNITS), 8)) as ex:
        list(ex.map(one, UNITS))


def resources(d):
    out = {}
    for fn in sorted(os.listdir(d)):
        if not fn.endswith(".remarks"):
            continue
        name = None
        for line in open(os.path.join(d, fn)):
            m = re.search(r"remark: .*?Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = {"file": fn[:-8]}
                continue
            m = re.search(r"remark: .*?\s{2,}([A-Za-z][^:]*): (\d+)", line)
            if m and name:
                out[name][m.group(1).strip()] = int(m.group(2))
    return out


def streams(d):
    out = {}
    for fn in sorted(os.listdir(d)):
        if not fn.endswith(".s"):
            continue
        name, body = None, []
        for line in open(os.path.join(d, fn)):
            m = re.match(r"^(_Z\w+):\s", line)
            if m and name is None:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end"):
                out[name] = normalise(name, body)
                name = None
                continue
            body.append(line)
    return out


def normalise(name, body):
    labels, res = {}, []

    def lab(m):
        return labels.setdefault(m.group(0), f".L{len(labels)}")

    for line in body:
        line = line.split(";")[0].rstrip()
        s = line.strip()
        if not s or s.startswith((".loc", ".file", ".cfi", ".p2align", "s_nop", "s_code_end", ".text", ".section")):
            continue
        line = line.replace(name, "KERNEL")
        res.append(re.sub(r"\.L(BB|tmp)\w+", lab, line))
    return res


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compare(a, b, renames=()):
    ra, rb, sa, sb = resources(a), resources(b), streams(a), streams(b)
    dm = demangle(sorted(set(ra) | set(rb)))
    for pair in renames:
        old, new = pair.split("=", 1)
        na = [n for n in ra if n not in rb and dm[n].startswith(old)]
        nb = [n for n in rb if n not in ra and dm[n].startswith(new)]
        if len(na) != 1 or len(nb) != 1:
            sys.exit(f"{pair}: {len(na)} kernels of A and {len(nb)} of B match")
        rb[na[0]], sb[na[0]] = rb.pop(nb[0]), sb.pop(nb[0], None)
        dm[na[0]] += f"  ->  {dm[nb[0]]}"
    names = sorted(set(ra) | set(rb))
    print("kernel | file A -> B | " + " | ".join(FIELDS) + " | same ISA")
    bad = 0
    for n in names:
        x, y = ra.get(n), rb.get(n)
        if x is None or y is None:
            print(f"{dm[n]} | only in {'A' if y is None else 'B'}")
            continue
        cols = [f"{x.get(f)}" if x.get(f) == y.get(f) else f"{x.get(f)} -> {y.get(f)}" for f in FIELDS]
        same = sa.get(n) == sb.get(n) and n in sa
        extra = ""
        if not same:  # how far apart: line counts and the change in the count of each mnemonic
            ca, cb = (Counter(ln.split()[0] for ln in s.get(n, []) if ln.startswith("\t")) for s in (sa, sb))
            delta = ", ".join(f"{k} {cb[k] - ca[k]:+d}" for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k])
            extra = f" ({len(sa.get(n, []))} -> {len(sb.get(n, []))} lines; {delta or 'same mnemonics, other order / registers'})"
        files = x["file"] if x["file"] == y["file"] else f"{x['file']} -> {y['file']}"
        print(f"{dm[n]} | {files} | " + " | ".join(cols) + f" | {'yes' if same else 'NO'}{extra}")
        worse = (y.get("ScratchSize [bytes/lane]", 0) > 0 and x.get("ScratchSize [bytes/lane]", 0) == 0) or \
            y.get("Occupancy [waves/SIMD]") < x.get("Occupancy [waves/SIMD]") or \
            y.get("LDS Size [bytes/block]") != x.get("LDS Size [bytes/block]")
        bad += bool(worse)
    print(f"kernels: {len(names)}; with new scratch, lost occupancy or another LDS size: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4:]))
