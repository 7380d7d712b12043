"""Host: bench.py's options and the --dump-outputs sampling (no GPU)."""
import numpy as np
import torch

import bench


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.steps == 5 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_rows_keeps_small_arrays_whole_and_samples_large_ones_the_same_way():
    cap = bench.DUMP_ARRAY_BYTES
    assert bench.dump_rows(cap // 4, 4) is None  # exactly at the cap: every row
    idx = bench.dump_rows(cap // 4 + 1, 4)
    assert len(idx) == cap // 4 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] <= cap // 4
    rows, row_bytes = 823_296, 48 * 4  # the observation tape of the default workload, as float32
    idx = bench.dump_rows(rows, row_bytes)
    assert len(idx) * row_bytes <= cap < (len(idx) + 1) * row_bytes
    assert np.array_equal(idx, bench.dump_rows(rows, row_bytes)) and len(np.unique(idx)) == len(idx)


def test_host_output_dtypes_and_sample():
    t = torch.arange(6, dtype=torch.bfloat16).reshape(3, 2)
    a = bench.host_output(t)
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(6, dtype=np.float32).reshape(3, 2))
    assert bench.host_output(torch.ones(4, dtype=torch.uint8)).dtype == np.float32
    assert bench.host_output(torch.ones(4, dtype=torch.float64)).dtype == np.float64
    n = bench.DUMP_ARRAY_BYTES // 8 + 5
    big = torch.arange(n, dtype=torch.float64)
    a = bench.host_output(big)
    assert a.nbytes <= bench.DUMP_ARRAY_BYTES and np.array_equal(a, bench.dump_rows(n, 8).astype(np.float64))
