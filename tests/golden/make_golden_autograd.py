#!/usr/bin/env python3
"""Records tests/golden/autograd_parent.npz on the device: what every public function of
trajectory_controller_amd.autograd returns -- outputs, the gradients of every differentiable input under a drawn
cotangent, the forward_ad tangents where forward mode exists -- for the cases of tests/model/autograd_parent_common.py
(n = 70, H = 4 and 7, 3 steps; inputs and recorded results only).  tests/test_autograd_parent_gpu.py holds the module
to the recording byte for byte.

    python tests/golden/make_golden_autograd.py [OUT.npz]

Every case is run twice, on two solvers; an array whose bytes differ between the two runs is named and left out.  The
committed recording was made at commit 98e286b ("Test the compact closed loop off the default vehicle, partial
arrays"), the parent of the change that folded the module's duplicated Functions, expansion and parsing; none differed.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.model import autograd_parent_common as ap  # noqa: E402
from trajectory_controller_amd import MpcSolver  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "autograd_parent.npz")
    gold, dropped = {}, []
    for H in ap.HORIZONS:
        with MpcSolver(horizon=H, device=0) as first, MpcSolver(horizon=H, device=0) as second:
            src = ap.Source(seed=H)
            for case in ap.case_names():
                res = ap.run_case(H, case, first, src)
                again = ap.run_case(H, case, second, ap.Source(gold=src.seen))
                assert set(res) == set(again), case
                for k, a in res.items():
                    if a.dtype == again[k].dtype and a.tobytes() == again[k].tobytes():
                        gold[k] = a
                    else:
                        dropped.append(k)
                print(f"H={H} {case}: {len(res)} results, {sorted(k.rsplit('/', 1)[1] for k in res)}")
            gold.update(src.seen)
    np.savez_compressed(path, **gold)
    print(f"{len(gold)} arrays, {os.path.getsize(path)} bytes; differed between two runs: {dropped or 'none'}")


if __name__ == "__main__":
    main()
