#!/usr/bin/env python3
"""Diagnostic: what the LANE_FMA coordinate-descent kernel (the headline family, fp64) costs outside its loop and per
iteration -- scripts/cd_cost.py's probe for LANE_FMA.  smo_iters = max_iter = K: the CD kernel runs at most K iterations and
publishes every instance itself, so the difference between K = 50 and K = 0 is the loop; K = 0 is set-up, the screen, the
record and the queue key.  The library's HIP events around the first launch (CD + queue order) are timed, best of R.
    python scripts/cd_cost_fma.py [H] [R]          (TPC_MPC_LIB selects the library, for A/B builds)
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import compact_inputs

H = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n = 262144
v, dy, dphi = (torch.from_numpy(a).cuda() for a in compact_inputs(H, n))
res = {}
for k in (0, 50, 0, 50):
    with MpcSolver(horizon=H, algo="lane_fma", smo_iters=k, max_iter=k) as s:
        s.set_profiling(True)
        best = 1e9
        for _ in range(R):
            s.solve_batch_compact(v, dy, dphi, want_flags=False)
            k1, k2, _ = s.last_kernel_times()
            best = min(best, k1)
        res[k] = min(res.get(k, 1e9), best)
        print(f"H={H} smo_iters=max_iter={k:2d}: CD + queue order {best * 1e3:7.1f} us   (PG publish-only pass {k2 * 1e3:6.1f} us)")
print(f"loop (K=50 - K=0): {(res[50] - res[0]) * 1e3:.1f} us; outside the loop: {res[0] * 1e3:.1f} us")
