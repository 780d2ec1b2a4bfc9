#!/usr/bin/env python3
"""Timing of the general-form forward (solve_batch_general from a fresh controller, the full control sequence out: what
trajectory_controller_amd.mpc_general runs) at dlib's eps 0.01 and at 1e-10, and of its backward pass
(tpc_mpc_solve_batch_general_backward, every gradient output), fp64, DEVICE memory.  One JSON line per case; medians of
--reps timed calls after --warmup untimed ones, measured with events on the launch stream.
usage: bench_grad.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import general_inputs

NAMES = ["A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets"]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for I, H, n in ((2, 20, 262144), (2, 40, 16384)):
        g = general_inputs(H, n, I=I)
        dev = [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).cuda() for k in NAMES]
        ctl = torch.zeros(H * I, n, dtype=torch.float64, device="cuda:0")
        with MpcSolver(horizon=H) as s:
            rec = dict(inputs=I, horizon=H, n=n)
            for eps in (0.01, 1e-10):
                def fwd():
                    ctl.zero_()
                    s.solve_batch_general(*dev, controls=ctl, inputs=I, eps=eps)
                rec[f"forward_ms_eps{eps:g}"], _ = timed(fwd, max(3, args.reps // 4) if eps < 0.01 else args.reps,
                                                         1 if eps < 0.01 else args.warmup)
            gbar = torch.randn(H * I, n, dtype=torch.float64, device="cuda:0")

            def bwd():
                s.solve_batch_general_backward(*dev, ctl, gbar, inputs=I, want_flags=False)
            rec["backward_ms"], rec["backward_min_ms"] = timed(bwd, args.reps, args.warmup)
            out = s.solve_batch_general_backward(*dev, ctl, gbar, inputs=I)
            rec["backward_flags"] = s.last_flags
            rec["max_kkt_residual"] = float(out["kkt_residual"].max())
            # bytes the backward moves at least: inputs + controls + dL/du read, outputs written, the per-step
            # workspace written twice and read twice (mpc_grad_model.h)
            slots = 4 + I
            rec["backward_min_bytes_per_instance"] = 8 * ((4 + 2 * I + 2 + 2 + 3 * I + 2 + 2 * H + 2 * H * I)
                                                          + (4 + 2 * I + 2 + 2 + 3 * I + 2 + 2 * H + 1)
                                                          + 4 * slots * H)
            rec["backward_GBps"] = rec["backward_min_bytes_per_instance"] * n / rec["backward_ms"] / 1e6
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
