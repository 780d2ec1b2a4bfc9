#!/usr/bin/env python3
"""Timing of the exact compact solve (tpc_mpc_solve_batch_compact_exact) with both fallback modes, beside its two
yardsticks on the same inputs in the same run: solve_batch_compact (AUTO, dlib's eps 0.01 -- dlib's answer, not the
optimum) and solve_batch_general (eps 0.01) + polish_batch_general on the expanded arrays (the optimum, the way a host
gets it without this entry; the expansion and its upload are not timed).  fp64, DEVICE memory.  One JSON line per
shape; medians of --reps timed calls after --warmup untimed ones, measured with events on the launch stream.  Each
line also holds the share that fell back, the rounds histogram of phase 1 and the largest distance between the two
routes to the optimum.
usage: bench_compact_exact.py [--reps 20] [--warmup 3] [--out profiles/r13_compact_exact_timing.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trajectory_controller_amd import MpcSolver, compact_general_form
from trajectory_controller_amd.autograd import _param_defaults
from trajectory_controller_amd.synth import compact_inputs

SHAPES = ((262144, 4), (262144, 10), (262144, 20), (16384, 40))   # (n, H)


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
    ap.add_argument("--max-rounds", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n, H in SHAPES:
        v, dy, dphi = (torch.from_numpy(a).cuda() for a in compact_inputs(H, n))
        kw = dict(tol=args.tol, max_rounds=args.max_rounds)
        with MpcSolver(horizon=H) as s:
            rec = dict(horizon=H, n=n, algo="auto", **kw)
            out = (torch.empty_like(v), torch.empty_like(v))
            rec["compact_eps0.01_ms"], _ = timed(
                lambda: s.solve_batch_compact(v, dy, dphi, want_flags=False, out=out), args.reps, args.warmup)
            dlib_front = out[0].clone()
            ins = [t.contiguous() for t in compact_general_form(v, dy, dphi, *_param_defaults(s.params), H).values()]
            ctl = torch.zeros(2 * H, n, dtype=torch.float64, device=v.device)

            def solve():
                ctl.zero_()
                s.solve_batch_general(*ins, controls=ctl, inputs=2)
            rec["general_eps0.01_ms"], _ = timed(solve, args.reps, args.warmup)

            def solve_polish():
                solve()
                s.polish_batch_general(*ins, ctl, inputs=2, want_status=False, **kw)
            rec["general_plus_polish_ms"], _ = timed(solve_polish, args.reps, args.warmup)
            torch.cuda.synchronize()
            ref_front = ctl[0].clone()
            for fallback in ("none", "solve"):
                rec[f"exact_{fallback}_ms"], rec[f"exact_{fallback}_min_ms"] = timed(
                    lambda: s.solve_batch_compact_exact(v, dy, dphi, fallback=fallback, want_status=False, **kw),
                    args.reps, args.warmup)
            front, rear, st, fell = s.solve_batch_compact_exact(v, dy, dphi, fallback="solve", **kw)
            rec["flags_solve"] = s.last_flags
            _, _, st1, _ = s.solve_batch_compact_exact(v, dy, dphi, fallback="none", **kw)
            rec["flags_none"] = s.last_flags
            torch.cuda.synchronize()
            ok = st >= 0
            rec["fell_back"] = int(fell.sum())
            rec["fell_back_share"] = float(fell.double().mean())
            rec["left_unverified"] = int((~ok).sum())
            rec["phase1_rounds_histogram"] = torch.bincount(st1[st1 >= 0], minlength=args.max_rounds + 1).tolist()
            rec["phase1_mean_rounds"] = float(st1[st1 >= 0].double().mean())
            rec["max_abs_front_exact_minus_general_polish"] = float((front - ref_front)[ok].abs().max())
            rec["max_abs_front_exact_minus_dlib_eps0.01"] = float((front - dlib_front)[ok].abs().max())
            rec["speedup_over_general_plus_polish"] = rec["general_plus_polish_ms"] / rec["exact_solve_ms"]
            rec["ratio_to_compact_eps0.01"] = rec["exact_solve_ms"] / rec["compact_eps0.01_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
