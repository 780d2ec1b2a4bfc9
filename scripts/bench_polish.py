#!/usr/bin/env python3
"""Timing of the polish of the general form (tpc_mpc_polish_batch_general) from an eps-0.01 LANE solve, beside
solve_batch_general with the full control sequence out at dlib's eps 0.01 and at eps 1e-10 on the same inputs in the
same run, fp64, DEVICE memory.  One JSON line per case; medians of --reps timed calls after --warmup untimed ones,
measured with events on the launch stream.  The polish is timed on a fresh copy of the loose sequence each call (the
copy is inside the timed region and is timed alone as copy_ms).
usage: bench_polish.py [--reps 20] [--warmup 3] [--out FILE]"""
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
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-rounds", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for I, H, n in ((2, 20, 262144), (2, 40, 16384)):
        g = general_inputs(H, n, I=I, seed=5)
        dev = [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).cuda() for k in NAMES]
        ctl = torch.zeros(H * I, n, dtype=torch.float64, device="cuda:0")
        with MpcSolver(horizon=H, algo="lane") as s:
            rec = dict(inputs=I, horizon=H, n=n, algo="lane", tol=args.tol, max_rounds=args.max_rounds)
            tight = None
            for eps in (1e-10, 0.01):   # eps 0.01 last: ctl then holds the loose sequence
                def fwd():
                    ctl.zero_()
                    s.solve_batch_general(*dev, controls=ctl, inputs=I, eps=eps)
                rec[f"solve_ms_eps{eps:g}"], _ = timed(fwd, max(3, args.reps // 4) if eps < 0.01 else args.reps,
                                                       1 if eps < 0.01 else args.warmup)
                rec[f"solve_flags_eps{eps:g}"] = s.last_flags
                if eps < 0.01:
                    tight = ctl.clone()
            loose = ctl.clone()
            work = torch.empty_like(loose)
            rec["copy_ms"], _ = timed(lambda: work.copy_(loose), args.reps, args.warmup)

            def pol():
                work.copy_(loose)
                s.polish_batch_general(*dev, work, tol=args.tol, max_rounds=args.max_rounds, inputs=I,
                                       want_status=False)
            rec["polish_ms"], rec["polish_min_ms"] = timed(pol, args.reps, args.warmup)
            work.copy_(loose)
            _, st, rin, rout = s.polish_batch_general(*dev, work, tol=args.tol, max_rounds=args.max_rounds, inputs=I)
            torch.cuda.synchronize()
            ok = st >= 0
            rec["polish_flags"] = s.last_flags
            rec["polished"] = int(ok.sum())
            rec["rounds_histogram"] = torch.bincount(st[ok]).tolist()
            rec["max_residual_in"] = float(rin.max())
            rec["max_residual_out_polished"] = float(rout[ok].max())
            rec["max_abs_loose_minus_tight"] = float((loose - tight).abs().max())
            rec["max_abs_polished_minus_tight"] = float((work - tight)[:, ok].abs().max())
            rec["solve_plus_polish_ms"] = rec["solve_ms_eps0.01"] + rec["polish_ms"] - rec["copy_ms"]
            rec["speedup_over_eps1e-10"] = rec["solve_ms_eps1e-10"] / rec["solve_plus_polish_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
