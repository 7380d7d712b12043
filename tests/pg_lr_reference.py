"""Pure-Python f64 restatement of the step-size controller of dxrl_pg_adam_step_ctl (the rules in
include/dxrl.h) and of the three learning-rate schedules.  Every operation is one IEEE f64
operation on Python floats, in the order the header states them, so a device run fed the same
(kl_sum, rows) must agree bit for bit."""
import math
import struct

SLOTS = ("applied", "skipped", "scale", "stopped", "stop_pass", "iter_applied", "iter_skipped", "lr_first",
         "lr_last", "kl_max", "kl_sum", "kl_rows")
INT_SLOTS = ("applied", "skipped", "stopped", "stop_pass", "iter_applied", "iter_skipped")
SLOT_WORDS = 16
COLUMNS = ("lr", "lr_last", "updates", "skipped", "stop_pass", "kl_max", "kl_epoch", "lr_scale")


def fresh_state():
    s = {k: (0 if k in INT_SLOTS else 0.0) for k in SLOTS}
    s["scale"], s["stop_pass"] = 1.0, -1
    return s


def control(lr_nominal, lr_min=1e-6, lr_max=1e-2, target_kl=0.0, stop_factor=1.5, adapt=0, adapt_factor=1.5,
            adapt_band=2.0, pass_index=0, last_epoch=1, last_pass=1):
    return dict(lr_nominal=float(lr_nominal), lr_min=float(lr_min), lr_max=float(lr_max), target_kl=float(target_kl),
                stop_factor=float(stop_factor), adapt=int(adapt), adapt_factor=float(adapt_factor),
                adapt_band=float(adapt_band), pass_index=int(pass_index), last_epoch=int(last_epoch),
                last_pass=int(last_pass))


def step(state, c, kl_sum, rows):
    """One call: (next state, decision, row).  decision = {"applied", "lr", "t"} (lr / t of an
    applied pass, None otherwise); row = the 8 columns of a last_pass call, else None."""
    kl_sum, rows = float(kl_sum), float(rows)
    first = c["pass_index"] == 0
    s = dict(state)
    if first:  # rule 1
        s.update(stopped=0, stop_pass=-1, iter_applied=0, iter_skipped=0, lr_first=0.0, lr_last=0.0, kl_sum=0.0,
                 kl_rows=0.0)
    kl = kl_sum / rows
    s["kl_max"] = kl if first or kl > state["kl_max"] else state["kl_max"]
    if c["target_kl"] > 0.0 and not s["stopped"] and kl > c["stop_factor"] * c["target_kl"]:  # rule 2
        s["stopped"], s["stop_pass"] = 1, c["pass_index"]
    decision = {"applied": not s["stopped"], "lr": None, "t": None, "kl": kl}
    if s["stopped"]:  # rule 3
        s["skipped"] += 1
        s["iter_skipped"] += 1
    else:  # rule 4
        lr = c["lr_nominal"] * state["scale"]
        lr = c["lr_min"] if lr < c["lr_min"] else (c["lr_max"] if lr > c["lr_max"] else lr)
        s["applied"] += 1
        s["iter_applied"] += 1
        if s["iter_applied"] == 1:
            s["lr_first"] = lr
        s["lr_last"] = lr
        decision.update(lr=lr, t=s["applied"])
    if c["last_epoch"]:  # rule 5
        s["kl_sum"] += kl_sum
        s["kl_rows"] += rows
    row = None
    if c["last_pass"]:
        kl_epoch = s["kl_sum"] / s["kl_rows"] if s["kl_rows"] > 0.0 else 0.0
        scale = state["scale"]
        if c["adapt"] and c["target_kl"] > 0.0 and s["kl_rows"] > 0.0:
            if kl_epoch > c["adapt_band"] * c["target_kl"]:
                scale = scale / c["adapt_factor"]
            elif kl_epoch < c["target_kl"] / c["adapt_band"]:
                scale = scale * c["adapt_factor"]
        if c["lr_nominal"] * scale > c["lr_max"]:
            scale = c["lr_max"] / c["lr_nominal"]
            if c["lr_nominal"] * scale > c["lr_max"]:
                scale = math.nextafter(scale, 0.0)
        elif c["lr_nominal"] * scale < c["lr_min"]:
            scale = c["lr_min"] / c["lr_nominal"]
            if c["lr_nominal"] * scale < c["lr_min"]:
                scale = math.nextafter(scale, math.inf)
        s["scale"] = scale
        row = [s["lr_first"], s["lr_last"], float(s["iter_applied"]), float(s["iter_skipped"]),
               float(s["stop_pass"]), s["kl_max"], kl_epoch, scale]  # rule 6
    return s, decision, row


def state_words(s):
    """The slot as the device holds it: SLOT_WORDS 64-bit words (int64 or the f64's bits)."""
    out = []
    for k in SLOTS:
        out.append(int(s[k]) if k in INT_SLOTS else struct.unpack("<q", struct.pack("<d", float(s[k])))[0])
    return out + [0] * (SLOT_WORDS - len(SLOTS))


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def schedule(kind, lr, lr_final, n, i):
    """lr at iteration 0, lr_final at iteration n and beyond."""
    lr = float(lr)
    if kind == "constant":
        return lr
    end = float(lr_final)
    if i <= 0:
        return lr
    if i >= n:
        return end
    if kind == "linear":
        return lr + (end - lr) * (i / n)
    if kind == "cosine":
        return end + 0.5 * (lr - end) * (1.0 + math.cos(math.pi * i / n))
    raise ValueError(kind)
