#!/usr/bin/env python3
"""Timing of the Newton-first closed loop (tpc_mpc_rollout_newton), fp64, two inputs, DEVICE memory, in one run on the
same inputs: rollout_polished at dlib's eps 0.01 (the yardstick: per step the solve dispatch and the fused polish +
step kernel) and rollout_newton with both fallback modes ("none": the one-launch Newton pass alone; "solve": plus
gather, rollout_polished's loop on the instances that left the pass, scatter).  Also the share of instances that fell
back, the distribution of first_unverified and the mean polish rounds per step.  One JSON line per case; medians of
--reps event-timed calls after --warmup untimed ones.
usage: bench_rollout_newton.py [--reps 20] [--warmup 3] [--out FILE]"""
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
CASES = ((16384, 20, 20), (65536, 10, 50), (262144, 20, 10))   # (n, H, steps): bench_rollout_polish.py's


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
        pol = dict(tol=args.tol, max_rounds=args.max_rounds)
        with MpcSolver(horizon=H) as s:
            rec = dict(inputs=I, horizon=H, steps=S, n=n, **pol)
            rec["rollout_polished_ms"], rec["rollout_polished_min_ms"] = timed(
                lambda: s.rollout_polished(S, *dev, inputs=I, want_status=False, **pol), args.reps, args.warmup)
            for fallback in ("none", "solve"):
                rec[f"rollout_newton_{fallback}_ms"], rec[f"rollout_newton_{fallback}_min_ms"] = timed(
                    lambda: s.rollout_newton(S, *dev, inputs=I, fallback=fallback, want_status=False, **pol),
                    args.reps, args.warmup)

            _, _, _, st, _, first = s.rollout_newton(S, *dev, inputs=I, fallback="none", **pol)
            torch.cuda.synchronize()
            rec["newton_none_flags"] = s.last_flags
            ok = st >= 0
            rec["fell_back"] = int((first < S).sum())
            rec["fell_back_share"] = float((first < S).double().mean())
            rec["first_unverified_histogram"] = torch.bincount(first, minlength=S + 1).tolist()
            rec["mean_rounds_per_step"] = [round(float(st[k][ok[k]].double().mean()), 3) for k in range(S)]
            _, _, _, st2, _, _ = s.rollout_newton(S, *dev, inputs=I, fallback="solve", **pol)
            torch.cuda.synchronize()
            rec["newton_solve_flags"] = s.last_flags
            rec["polished_share_after_fallback"] = float((st2 >= 0).double().mean())
            rec["polished_over_newton_solve"] = rec["rollout_polished_ms"] / rec["rollout_newton_solve_ms"]
            rec["polished_over_newton_none"] = rec["rollout_polished_ms"] / rec["rollout_newton_none_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
