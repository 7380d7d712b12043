"""Per-step segment cycles of the PG rollout (diagnostic only): DIAG=128 -> k_pg_rollout_ws
stamps, one record per wave (s0 obs row, s1 L1, s2 L2, s3 head phase, s4 head barrier wait, s5 P4,
s6 P4 barrier), at ENVS >= 32 per CU (or DIAG | 1024) the 32-env k_pg_rollout_e8.  Configs: easy,
hard, variable + fused noise 0.05 (C5's).

    python tools/rollout_stamps.py            measure (in a child process), then print the tables
    python tools/rollout_stamps.py --raw      measure only: the library's own lines
    python tools/rollout_stamps.py --parse F  tables of an earlier run's log

A stamp k is taken BEFORE the barrier that closes its phase, except s4 and s6, which are the waits
at the head-phase and end-of-step barriers.  So a wave's s3 / s5 is its own work in the phase (plus
its wait at the barrier before the phase), and the phase lasts as long as its longest wave: the
table prints every wave's cycles per segment, the maximum and the wave that sets it."""
import os
import re
import subprocess
import sys

SEGMENTS = ("s0 obs row", "s1 L1", "s2 L2", "s3 head phase", "s4 head wait", "s5 P4", "s6 P4 wait")
_WAVE = re.compile(r"^\s*wave (\d+):((?: s\d+=\d+)+)\s*$")
_MEAN = re.compile(r"^rollout_\w+ (env|aux) cycles/step:")
_SEG = re.compile(r"s(\d+)=(\d+)")


def parse_stamps(text):
    """{config title: {wave: [cycles of s0, s1, ...]}} of the library's diag-128 lines.  A title
    is the line the measuring loop prints before a config's rollout ("easy", "variable noise");
    lines that are neither a title, a mean nor a wave record (driver chatter) are skipped."""
    out, title = {}, None
    for line in text.splitlines():
        m = _WAVE.match(line)
        if m:
            if title is None:
                title = "?"
            segs = sorted((int(k), int(v)) for k, v in _SEG.findall(m.group(2)))
            if [k for k, _ in segs] != list(range(len(segs))):
                raise ValueError(f"segments out of order: {line!r}")
            out.setdefault(title, {})[int(m.group(1))] = [v for _, v in segs]
        elif _MEAN.match(line) or not line.strip() or "/" in line or ":" in line:
            continue
        elif len(line.split()) <= 2:
            title = " ".join(line.split())
    return out


def table(waves):
    """Rows: segments; columns: the waves, the maximum and the wave that sets it."""
    ids = sorted(waves)
    nseg = min(len(waves[w]) for w in ids)
    lines = ["segment        " + "".join(f"{'w' + str(w):>7}" for w in ids) + "    max  wave"]
    for k in range(nseg):
        vals = [waves[w][k] for w in ids]
        top = max(vals)
        name = SEGMENTS[k] if k < len(SEGMENTS) else f"s{k}"
        lines.append(f"{name:<15}" + "".join(f"{v:>7}" for v in vals) + f"{top:>7}  {ids[vals.index(top)]:>4}")
    lines.append(f"{'sum':<15}" + "".join(f"{sum(waves[w][:nseg]):>7}" for w in ids))
    return "\n".join(lines)


def report(text):
    return "\n\n".join(f"{title}\n{table(waves)}" for title, waves in parse_stamps(text).items())


def measure():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import dexterous_rl_manipulation_amd as pkg
    from dexterous_rl_manipulation_amd import envs, trainer

    for cur, noise in (("easy", 0.0), ("hard", 0.0), ("variable", 0.05)):
        env = envs.VecEnv(int(os.environ.get("ENVS", "4096")), curriculum_config=pkg.CurriculumConfig.named(cur), reward_type="dense", seed=1,
                          device=torch.device("cuda:0"))
        tr = trainer.PGTrainer(env, trainer.TrainerConfig(horizon=200, seed=7, obs_noise_std=noise, dyn_noise_std=noise))
        env.reset(write_obs=False)
        tr.rollout()
        tr.diag_flags = int(os.environ.get("DIAG", "128"))
        print(cur, "noise" if noise else "", file=sys.stderr, flush=True)
        tr.rollout()
        torch.cuda.synchronize()
        tr.diag_flags = 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--raw"]:
        measure()
    elif sys.argv[1:2] == ["--parse"]:
        print(report(open(sys.argv[2]).read()))
    else:
        raw = subprocess.run([sys.executable, os.path.abspath(__file__), "--raw"], stderr=subprocess.PIPE, text=True, check=True).stderr
        print(raw)
        print(report(raw))
