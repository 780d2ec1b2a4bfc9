#!/usr/bin/env python3
"""Timing of the polished closed loop (tpc_mpc_rollout_polished), fp64, two inputs, DEVICE memory, in one run on the
same inputs: rollout_record at dlib's eps 0.01 and at eps 1e-10 (the two routes without the polish), rollout_polished
at eps 0.01 (solve dispatch + the fused polish + step kernel per step), and the unfused composition -- per step
solve_batch_general carrying controls and v, polish_batch_general, then the plant update and the target shift as torch
operations on the device.  Also the mean solver iterations per step with and without the polish, the share of
polished (instance, step) pairs and the largest residual out.  One JSON line per case; medians of --reps event-timed
calls after --warmup untimed ones (the eps-1e-10 route: a quarter of the reps, one warm-up).
usage: bench_rollout_polish.py [--reps 20] [--warmup 3] [--out FILE]"""
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
CASES = ((16384, 20, 20), (65536, 10, 50), (262144, 20, 10))   # (n, H, steps): profiles/r07_rollout_grad_timing.jsonl's


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
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--max-rounds", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    I = 2
    lines = []
    for n, H, S in CASES:
        g = general_inputs(H, n, I=I, seed=5)
        dev = [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).cuda() for k in NAMES]
        A, B, Cc = dev[0], dev[1], dev[2]
        pol = dict(tol=args.tol, max_rounds=args.max_rounds)
        with MpcSolver(horizon=H) as s:
            rec = dict(inputs=I, horizon=H, steps=S, n=n, **pol)
            slow = max(3, args.reps // 4)
            rec["rollout_record_ms_eps1e-10"], _ = timed(lambda: s.rollout_record(S, *dev, inputs=I, eps=1e-10), slow, 1)
            rec["rollout_record_flags_eps1e-10"] = s.last_flags
            rec["rollout_record_ms_eps0.01"], _ = timed(lambda: s.rollout_record(S, *dev, inputs=I), args.reps, args.warmup)
            rec["rollout_polished_ms"], rec["rollout_polished_min_ms"] = timed(
                lambda: s.rollout_polished(S, *dev, inputs=I, want_status=False, **pol), args.reps, args.warmup)

            def composed():
                c = torch.zeros(H * I, n, dtype=torch.float64, device="cuda:0")
                v = torch.zeros_like(c)
                x, T = dev[7].clone(), dev[8].clone()
                for _ in range(S):
                    s.solve_batch_general(*dev[:7], x, T, controls=c, v_state=v, inputs=I)
                    s.polish_batch_general(*dev[:7], x, T, c, inputs=I, want_status=False, **pol)
                    x = torch.stack([A[0] * x[0] + A[1] * x[1] + (B[0] * c[0] + B[1] * c[1]) + Cc[0],
                                     A[2] * x[0] + A[3] * x[1] + (B[2] * c[0] + B[3] * c[1]) + Cc[1]])
                    T = torch.cat([T[2:], T[-2:]])
            rec["composed_ms"], rec["composed_min_ms"] = timed(composed, args.reps, args.warmup)

            _, _, _, it0 = s.rollout_record(S, *dev, inputs=I, want_iters=True)
            ri, ro = (torch.empty(S, n, dtype=torch.float64, device="cuda:0") for _ in range(2))
            _, _, _, st, it1 = s.rollout_polished(S, *dev, inputs=I, want_iters=True, residuals=(ri, ro), **pol)
            torch.cuda.synchronize()
            ok = st >= 0
            rec["rollout_polished_flags"] = s.last_flags
            rec["mean_iters_per_step_unpolished"] = [round(float(v), 2) for v in it0.double().mean(dim=1)]
            rec["mean_iters_per_step_polished"] = [round(float(v), 2) for v in it1.double().mean(dim=1)]
            rec["polished_pairs"] = int(ok.sum())
            rec["pairs"] = int(ok.numel())
            rec["polished_share"] = float(ok.double().mean())
            rec["rounds_histogram"] = torch.bincount(st[ok]).tolist()
            rec["max_residual_in"] = float(ri.max())
            rec["max_residual_out_polished"] = float(ro[ok].max())
            rec["polished_over_record_pct"] = 100.0 * (rec["rollout_polished_ms"] / rec["rollout_record_ms_eps0.01"] - 1.0)
            rec["eps1e-10_over_polished"] = rec["rollout_record_ms_eps1e-10"] / rec["rollout_polished_ms"]
            rec["fused_over_composed"] = rec["rollout_polished_ms"] / rec["composed_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
