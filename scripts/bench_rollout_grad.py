#!/usr/bin/env python3
"""Timing of the closed loop's forward and backward, fp64, two inputs, DEVICE memory: rollout against rollout_record
(interleaved pairs, the same inputs), the fused backward (tpc_mpc_rollout_backward, every gradient output, dL/dcontrols
and dL/dstates given) and, measured in the same run, steps x the single-solve backward
(tpc_mpc_solve_batch_general_backward) at the same (n, H, I) -- what chaining the single solve's backward step by step
would cost in kernel time alone.  One JSON line per case; medians of --reps event-timed calls after --warmup untimed
ones.
usage: bench_rollout_grad.py [--reps 20] [--warmup 3] [--out FILE]"""
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
CASES = ((16384, 20, 20), (65536, 10, 50), (262144, 20, 10))   # (n, H, steps)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    I = 2
    for n, H, S in CASES:
        g = general_inputs(H, n, I=I)
        dev = [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).cuda() for k in NAMES]
        last = dev[8][2 * (H - 1):2 * H]
        nlt = (last.repeat(S, 1) + 0.01 * torch.randn(2 * S, n, dtype=torch.float64, device="cuda:0")).contiguous()
        gu = torch.randn(S * I, n, dtype=torch.float64, device="cuda:0")
        gx = torch.randn(2 * S, n, dtype=torch.float64, device="cuda:0")
        with MpcSolver(horizon=H) as s:
            rec = dict(inputs=I, horizon=H, steps=S, n=n)
            _, states, seqs, _ = s.rollout_record(S, *dev, nlt, inputs=I)
            fwd = lambda: s.rollout(S, *dev, nlt, inputs=I)
            fwd_rec = lambda: s.rollout_record(S, *dev, nlt, inputs=I)
            for _ in range(args.warmup):
                fwd()
                fwd_rec()
            reps_f = max(3, args.reps // 4)
            a, b = [], []
            for _ in range(reps_f):   # interleaved, so drift hits both alike
                a.append(timed(fwd))
                b.append(timed(fwd_rec))
            rec["rollout_ms"], rec["rollout_record_ms"] = float(np.median(a)), float(np.median(b))
            rec["record_overhead_pct"] = 100.0 * (rec["rollout_record_ms"] / rec["rollout_ms"] - 1.0)

            bwd = lambda: s.rollout_backward(S, *dev, nlt, sequences=seqs, states=states, grad_controls=gu,
                                             grad_states=gx, inputs=I, want_flags=False)
            ctl = seqs[(S - 1) * H * I:].contiguous()
            gbar = torch.randn(H * I, n, dtype=torch.float64, device="cuda:0")
            one = lambda: s.solve_batch_general_backward(*dev, ctl, gbar, inputs=I, want_flags=False)
            for _ in range(args.warmup):
                bwd()
                one()
            a, b = [], []
            for _ in range(args.reps):
                a.append(timed(bwd))
                b.append(timed(one))
            rec["fused_backward_ms"], rec["fused_backward_min_ms"] = float(np.median(a)), float(np.min(a))
            rec["single_backward_ms"] = float(np.median(b))
            rec["steps_x_single_backward_ms"] = S * rec["single_backward_ms"]
            rec["fused_vs_chained"] = rec["fused_backward_ms"] / rec["steps_x_single_backward_ms"]
            out = s.rollout_backward(S, *dev, nlt, sequences=seqs, states=states, grad_controls=gu, grad_states=gx,
                                     inputs=I)
            rec["backward_flags"] = s.last_flags
            rec["max_kkt_residual"] = float(out["kkt_residual"].max())
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del dev, states, seqs, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
