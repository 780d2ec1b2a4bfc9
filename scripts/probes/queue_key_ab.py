#!/usr/bin/env python3
"""Probe (GPU): the table-predicted queue key of LANE_FMA fp64 N = 20 on and off (tpc_mpc_x_set_queue_key), interleaved in one
process on one box: kernel times (cd, pg) and lane statistics per solve, results compared bit for bit.

    [TPC_MPC_LIB=ab/NAME/libtpc_mpc.so] python scripts/probes/queue_key_ab.py [rounds] [n] [algo]

With TPC_MPC_LIB a variant build runs instead (scripts/build_asm_variant.sh: the stop test's check positions)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import compact_inputs

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
algo = sys.argv[3] if len(sys.argv) > 3 else "auto"
H = 20
tv, ty, tp = (torch.from_numpy(a).cuda() for a in compact_inputs(H, n))
s = MpcSolver(horizon=H, algo=algo)
s.set_profiling(True)
f0, r0, it0 = s.solve_batch_compact(tv, ty, tp, want_iters=True)
pg_iters = float((it0.double() - 50).clamp(min=0).sum())
res = {True: [], False: []}
for rnd in range(rounds):
    for on in (False, True):
        s.set_queue_key(on)
        f, r, it = s.solve_batch_compact(tv, ty, tp, want_iters=True)
        k1, k2, a = s.last_kernel_times()
        wi, rb = s.last_lane_stats()
        same = bool(torch.equal(f, f0) and torch.equal(r, r0) and torch.equal(it, it0))
        res[on].append((k1, k2, wi))
        print(f"round {rnd} key {s.last_queue_key():6s}: cd {k1:.4f} ms  pg {k2:.4f} ms  wave_iterations {wi}  refills {rb}  algo {a}  bits equal {same}")
for on in (False, True):
    a = np.array(res[on][1:] or res[on])   # (the first round warms up)
    print(f"n {n} {algo} key {'table ' if on else 'lambda'}: pg min {a[:, 1].min():.4f} median {np.median(a[:, 1]):.4f} max {a[:, 1].max():.4f} ms;"
          f"  cd min {a[:, 0].min():.4f} median {np.median(a[:, 0]):.4f} max {a[:, 0].max():.4f} ms;  wave_iterations median {np.median(a[:, 2]):.0f}"
          f"  lane utilisation {pg_iters / (64.0 * np.median(a[:, 2])):.4f}")
