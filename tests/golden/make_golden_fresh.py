#!/usr/bin/env python3
"""The real reference solver's answers for the "fresh" inputs of test_oracle_vs_live_dlib, generated
exactly like make_golden.py (real dlib::mpc compiled from the reference tree by oracle/Makefile; data
only, no reference source text), so that the test holds the restatement to real dlib on those inputs
where no real-dlib build exists.

    python tests/golden/make_golden_fresh.py

  compact_fresh.npz   for H in {4, 10, 20}: instances 5000 .. 5511 of the horizon-H synthetic stream
                      (v_H, dy_H, dphi_H) -> front_H, rear_H (reference weights, default eps / max_iter)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.bindings import DlibRef  # noqa: E402
from trajectory_controller_amd.synth import compact_inputs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
HORIZONS = (4, 10, 20)
FIRST, COUNT = 5000, 512


def main():
    ref = DlibRef()
    sets = {}
    for H in HORIZONS:
        v, dy, dphi = compact_inputs(H, COUNT, first=FIRST)
        f, r = ref.solve_compact(H, v, dy, dphi, nthreads=4)
        sets.update({f"v_H{H}": v, f"dy_H{H}": dy, f"dphi_H{H}": dphi, f"front_H{H}": f, f"rear_H{H}": r})
    np.savez_compressed(os.path.join(OUT, "compact_fresh.npz"), **sets)


if __name__ == "__main__":
    main()
