#!/usr/bin/env python3
"""Records tests/golden/newton_rounds_parent.npz: inputs and outputs of tpc_mpc_polish_batch_general (I = 1, 2) and of
tpc_mpc_solve_batch_compact_exact (cold, rows, warm) on the CPU host path of a host-only handle, at horizons 1, 4, 5, 6,
n = 67, with each entry's default round limit and with max_rounds = 1 (tests/model/newton_rounds_common.py has the
shapes and the runners; tests/test_newton_rounds_host.py and tests/test_newton_rounds_gpu.py hold the library to the
recording bit for bit).

The committed recording was made with the library built from commit 54064d7 ("Bind MpcSolver's arrays in one helper;
one GeneralIO builder, one tail"), the last one in which polish::polish_instance and cexact::exact_instance each carried
their own copy of the Newton rounds: build that commit's library and name it in TPC_MPC_LIB.  Run against any later
library, the script records that library instead -- which is only right for a deliberate change of the arithmetic.

Inputs: the polish's models are tests/model/mpc_grad_dense.mixed_batch (tight boxes, a pinned input); its starts are
random sequences reaching outside every box, with every third instance started at its own optimum.  The compact cases
take compact_inputs with a few zero targets (optimal at U = 0), the tight "asymmetric" and the "pinned" model of
compact_exact_common.VARIANTS, the "all" recipe of compact_rows_common with its boxes narrowed, a pinned rear input in
every seventh instance and compact_rows_common's invalid columns, and the mixed starts of compact_warm_common.
usage: TPC_MPC_LIB=/path/to/parent/libtpc_mpc.so python scripts/record_newton_rounds.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tests.model import compact_rows_common as cr
from tests.model import compact_warm_common as cw
from tests.model import mpc_grad_dense as dense
from tests.model import newton_rounds_common as nr
from tests.model.compact_exact_common import NAMES, VARIANTS
from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import compact_inputs

N, LD = nr.N, nr.LD
NONFINITE, BAD_MODEL = 5, 65          # the polish's flagged instances: first wavefront, and one of the last three lanes
SPOILED = (2, 9, 17, 25, 33, 41, 66)  # where compact_rows_common.INVALID's seven cases sit


def wide(a, pad=np.nan):
    w = np.full((a.shape[0], LD), pad)
    w[:, :N] = a
    return w


def polish_case(s, I, H):
    th = dense.mixed_batch(I, H, N, seed=3)
    if I == 1:
        th["lo"][::7, 0] = th["hi"][::7, 0] = 0.01          # mixed_batch pins an input only with I = 2
    th["targets"][NONFINITE, H - 1, 1] = np.inf
    th["R"][BAD_MODEL, I - 1] = 0.0
    ins = {k: wide(dense.soa(th[k], N)) for k in NAMES}
    start = np.random.default_rng(100 * H + I).uniform(-0.6, 0.6, (H * I, N))
    ins["controls"] = wide(start, nr.SENTINEL)
    # every third instance starts where the default call ends: verified in round 0
    first = nr.run_polish(s, I, H, ins, nr.POLISH_ROUNDS[0])
    done = np.flatnonzero((first["status"][:N] >= 0) & (np.arange(N) % 3 == 0))
    ins["controls"][:, done] = first["controls"][:, done]
    return ins


def compact_case(s, entry, H):
    v, dy, dphi = (a.copy() for a in compact_inputs(H, N, seed=0xC0DE + H))
    dy[::8] = dphi[::8] = 0.0                                # optimal at U = 0 where 0 is in the box
    ins = dict(v=v, dy=dy, dphi=dphi)
    if entry.endswith("rows"):
        rows = cr.recipe_rows("all", H, N)
        rows[cr.LO], rows[cr.HI] = 0.15 * rows[cr.LO], 0.15 * rows[cr.HI]
        rows[7, ::7] = rows[9, ::7] = 0.02
        ins["params_rows"], ins["v"] = cr.spoil(rows, v, SPOILED)
    else:
        variant = VARIANTS["pinned" if entry == "cold_pinned" else "asymmetric"]
        ins["lower"], ins["upper"] = np.array(variant["lower"]), np.array(variant["upper"])
        ins["v"][NONFINITE], ins["dphi"][BAD_MODEL] = np.nan, -np.inf      # both non-finite: a shared model has no 0x4
    if entry.startswith("warm"):
        # the sequences of a model one optimiser step away, a quarter of them without a start, a quarter random
        scale = 1.0 + 0.01 * cw.SIGNS
        before = dict(ins)
        if "params_rows" in ins:
            before["params_rows"] = ins["params_rows"].copy()
            before["params_rows"][cr.W] *= scale[:, None]
            previous = nr.run_compact(s, before, nr.COMPACT_ROUNDS[0])["sequence"]
        else:
            p = s.params
            weights = {w: getattr(p, w) * f for w, f in zip(cw.WEIGHTS, scale)}
            with MpcSolver(horizon=H, device=None, **weights) as moved:
                previous = nr.run_compact(moved, before, nr.COMPACT_ROUNDS[0])["sequence"]
        ins["start"] = cw.mixed_start(previous, H, 7 + H)
    return ins


def main():
    gold = {}
    for H in nr.HS:
        with MpcSolver(horizon=H, device=None) as s:
            for I in nr.INPUTS:
                case, ins = f"polish_I{I}_H{H}", polish_case(s, I, H)
                gold.update({f"{case}/in/{k}": a for k, a in ins.items()})
                for rounds in nr.POLISH_ROUNDS:
                    out = nr.run_polish(s, I, H, ins, rounds)
                    gold.update({f"{case}/r{rounds}/{k}": out[k] for k in nr.POLISH_OUT})
            for entry in nr.COMPACT:
                case, ins = f"{entry}_H{H}", compact_case(s, entry, H)
                gold.update({f"{case}/in/{k}": a for k, a in ins.items()})
                for rounds in nr.COMPACT_ROUNDS:
                    out = nr.run_compact(s, ins, rounds)
                    gold.update({f"{case}/r{rounds}/{k}": out[k] for k in nr.COMPACT_OUT})
    path = os.path.join(ROOT, "tests", "golden", "newton_rounds_parent.npz")
    np.savez_compressed(path, **gold)
    gold = np.load(path)
    for family, cases in nr.families().items():
        st = np.concatenate([gold[f"{c}/r{r[0]}/status"][:N] for c, r in cases])
        one = np.concatenate([gold[f"{c}/r{r[1]}/status"][:N] for c, r in cases])
        print(f"{family}: status histogram from -1 {np.bincount(st + 1).tolist()}, with one round "
              f"{np.bincount(one + 1).tolist()}")
    nr.check_contents(gold)
    print(f"{path}: {len(gold.files)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
