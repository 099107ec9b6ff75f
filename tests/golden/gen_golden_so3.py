#!/usr/bin/env python3
"""Generate the edge-rotation bundle-adjustment vectors (ba_so3_<case>.npz) from the high-precision model tests/so3_model.py.

Unlike gen_golden.py / gen_golden_loss.py this needs no reference: the cases are built deterministically by so3_model.case and everything
stored is the model's own result (mpmath at 60 digits, Jacobians by central differences), rounded to float64 once.  Per case:

  stored once      K, poses0, points0, obs (NaN = missing), angles, lam; e [W,N,2], Jp [W,N,2,6], Jl [W,N,2,3] (zero where nothing is observed)
  stored per loss  <tag>__cost, Hpp, gp, Hll, gl, S (upper triangle, row-major: the model's S is symmetric to the last bit), rhs, dposes,
                   dpoints at lam = 1e-3; tags huber, linear, soft_l1, cauchy, arctan (C = 1) and huber_c2.5 (C = 2.5)

tests/test_so3_model.py regenerates every file in memory and compares bit for bit; the GPU tests read the files through so3_model.load.

Usage:  python tests/golden/gen_golden_so3.py [case ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import so3_model as sm  # noqa: E402


if __name__ == "__main__":
    for name in (sys.argv[1:] or sm.CASES):
        fx = sm.build_fixture(name)
        np.savez_compressed(sm.path(name), **fx)
        print("wrote", sm.path(name), os.path.getsize(sm.path(name)), "bytes; costs",
              {tag: float(fx[tag + "__cost"]) for tag, _, _ in sm.LOSS_RUNS}, flush=True)
