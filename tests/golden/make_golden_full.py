#!/usr/bin/env python3
"""Golden vectors on FULL 2x2 models (tests/model/full_models.py: every entry of A and B live), generated from the
REAL reference solver exactly like make_golden_r02.py (real dlib::mpc compiled by oracle/Makefile; data only, no
reference source text).  The earlier fixtures all carry A = [1, Tv; 0, 1]; these pin the oracle off that structure.

    python tests/golden/make_golden_full.py

  general_full_I{1,2}_H{4,5,10,20,30,40}.npz   cold solves, n = 96 up to H = 20 and 48 above
  rollout_full_I{1,2}_H{4,5,10,20,30,40}.npz   12 controllers x 5 warm-started closed-loop steps each, per-instance
                                               models, set_last_target every step
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.bindings import DlibRef  # noqa: E402
from tests.model.full_models import NAMES, full_models, new_last_targets  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
HORIZONS = (4, 5, 10, 20, 30, 40)


def main():
    ref = DlibRef()
    for I in (1, 2):
        for H in HORIZONS:
            n = 96 if H <= 20 else 48
            g = full_models(I, H, n, seed=1)
            u0 = ref.solve_general(I, H, *[g[k] for k in NAMES])
            np.savez_compressed(os.path.join(OUT, f"general_full_I{I}_H{H}.npz"), u0=u0, **g)
            print(f"general_full I={I} H={H}: n={n} |u0| max {np.abs(u0).max():.4f}")
    steps, n = 5, 12
    for I in (1, 2):
        for H in HORIZONS:
            g = full_models(I, H, n, seed=2)
            nlt = new_last_targets(g, steps, seed=64 * I + H)
            controls = np.empty((n, steps, I))
            states = np.empty((n, steps, 2))
            for k in range(n):
                controls[k], states[k] = ref.rollout(I, H, steps, *[g[key][k] for key in NAMES], nlt[k])
            np.savez_compressed(os.path.join(OUT, f"rollout_full_I{I}_H{H}.npz"), controls=controls, states=states,
                                new_last_targets=nlt, steps=steps, **g)
            print(f"rollout_full I={I} H={H}: |u| max {np.abs(controls).max():.4f} |x| max {np.abs(states).max():.4f}")


if __name__ == "__main__":
    main()
