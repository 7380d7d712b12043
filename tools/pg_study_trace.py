"""For rocprofv3 --kernel-trace: dxrl_pg_runs_summarize on slabs of the study's size (12 runs x 200
rows x 24 columns and 12 x 11 x 16; 3 specs, 4 groups, 6 contrasts), 50 calls each."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexterous_rl_manipulation_amd import ablation, training_study as T  # noqa: E402

dev = torch.device("cuda:0")
arms = [a.name for a in ablation.pg_component_arms()]
off, flat = T.csr_groups([[a * 3 + k for k in range(3)] for a in range(4)])
weights = T.contrast_matrix(arms, ablation.PG_COMPONENT_CONTRASTS)
specs = ablation.pg_study_specs(3, 0.5, 3)
rng = np.random.default_rng(0)
for name, rows in (("training", 200), ("validation", 11)):
    cols = T._SLAB_COLS[name]
    slab = torch.from_numpy(rng.random((12, rows, cols))).to(dev)
    nat = T.native_specs(specs, name)
    for _ in range(50):
        pending, _n = T.summarize_device(slab, [rows] * 12, nat, off, flat, weights)
    torch.cuda.synchronize()
print("done")
