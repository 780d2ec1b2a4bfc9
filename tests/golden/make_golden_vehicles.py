#!/usr/bin/env python3
"""Golden vectors of the compact form OFF the reference controller's parameter set (tests/model/vehicles.py: other
weights, step sizes and wheelbases -- negative ones too --, weight_phi = 0, unequal bounds, a box that does not contain
u = 0, and speeds of both signs with one v = 0), generated from the REAL reference solver like make_golden_full.py
(real dlib::mpc compiled by oracle/Makefile; data only, no reference source text).  The compact_H*.npz fixtures all
carry the default vehicle and v > 0; these pin the oracle off that point.

    python tests/golden/make_golden_vehicles.py

  compact_vehicles_H{4,5,10,20,30,40}.npz   v, dy, dphi [48]: the first 48 instances of vehicles.inputs(H, .), and per
                                            vehicle allowed at that horizon front_<name>, rear_<name> [48]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.bindings import DlibRef  # noqa: E402
from tests.model import vehicles as vh  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
N = 48


def main():
    ref = DlibRef()
    for H in vh.HORIZONS:
        v, dy, dphi = vh.inputs(H, N)
        out = dict(v=v, dy=dy, dphi=dphi)
        for name in vh.names_at(H):
            out[f"front_{name}"], out[f"rear_{name}"] = ref.solve_compact(H, v, dy, dphi, **vh.oracle_kw(name))
        np.savez_compressed(os.path.join(OUT, f"compact_vehicles_H{H}.npz"), **out)
        print(f"compact_vehicles H={H}: {len(vh.names_at(H))} vehicles, {int((v < 0).sum())} of {N} speeds negative")


if __name__ == "__main__":
    main()
