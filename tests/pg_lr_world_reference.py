"""The sharded form of the step-size controller (dxrl_pg_adam_step_ctl_world, include/dxrl.h): the
ranks' (kl_sum, rows) records merged sequentially in rank order, then tests/pg_lr_reference.py's
step, by import -- the rules are stated there and nowhere else."""
import pg_lr_reference as R

RECORD_WORDS = 2


def merge(records):
    """(kl_sum, rows) of all ranks: ((r0 + r1) + r2) ... in rank order, one IEEE f64 add each."""
    records = [(float(k), float(n)) for k, n in records]
    assert records, "world >= 1"
    kl_sum, rows = records[0]
    for k, n in records[1:]:
        kl_sum = kl_sum + k
        rows = rows + n
    return kl_sum, rows


def step_world(state, c, records):
    return R.step(state, c, *merge(records))


def column_sum(col):
    """block_sum_partials' fixed order on a 256-thread workgroup (csrc/dxrl_pg.hip): thread t adds
    col[t], col[t + 256], ... in that order starting from 0.0; an xor butterfly over offsets 32, 16,
    .. 1 inside each 64-lane wave; then the four wave sums in wave order."""
    s = [0.0] * 256
    for k, v in enumerate(col):
        s[k % 256] = s[k % 256] + float(v)
    for o in (32, 16, 8, 4, 2, 1):
        s = [s[t] + s[(t & ~63) | ((t & 63) ^ o)] for t in range(256)]
    return ((s[0] + s[64]) + s[128]) + s[192]
