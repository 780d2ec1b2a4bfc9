#!/usr/bin/env python3
"""Timing of the closed loop's forward-mode derivative, fp64, two inputs, DEVICE memory, on the shapes of
profiles/r07_rollout_grad_timing.jsonl: rollout_forward (tpc_mpc_rollout_forward, tcontrols and tstates) with K = 1
and K = 4 directions (tangents of Q and R, the four weights), the fused backward (tpc_mpc_rollout_backward, every
gradient output) on the same recorded loop as the yardstick, and the steps * (I + 2) backward calls that give the same
Jacobian as the K = 4 call (one per output row, actually run).  Everything in one run, the three single calls
interleaved; one JSON line per case; medians of --reps event-timed calls after --warmup untimed ones.
usage: bench_rollout_tangent.py [--reps 20] [--warmup 3] [--out FILE]"""
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
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device="cuda:0")
    for n, H, S in CASES:
        g = general_inputs(H, n, I=I)
        dev = [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).cuda() for k in NAMES]
        last = dev[8][2 * (H - 1):2 * H]
        nlt = (last.repeat(S, 1) + 0.01 * rnd(2 * S, n)).contiguous()
        gu, gx = rnd(S * I, n), rnd(2 * S, n)
        with MpcSolver(horizon=H) as s:
            rec = dict(inputs=I, horizon=H, steps=S, n=n)
            _, states, seqs, *_ = s.rollout_newton(S, *dev, nlt, inputs=I, want_status=False)
            tan = {k: {"Q": rnd(k, 2, n), "R": rnd(k, I, n)} for k in (1, 4)}
            fwd = {k: (lambda k=k: s.rollout_forward(S, *dev, nlt, sequences=seqs, states=states, tangents=tan[k],
                                                     inputs=I, want_flags=False)) for k in (1, 4)}
            bwd = lambda: s.rollout_backward(S, *dev, nlt, sequences=seqs, states=states, grad_controls=gu,
                                             grad_states=gx, inputs=I, want_flags=False)
            for _ in range(args.warmup):
                fwd[1](), fwd[4](), bwd()
            a, b, c = [], [], []
            for _ in range(args.reps):   # interleaved, so drift hits all alike
                a.append(timed(fwd[1]))
                b.append(timed(fwd[4]))
                c.append(timed(bwd))
            rec["forward_k1_ms"], rec["forward_k4_ms"] = float(np.median(a)), float(np.median(b))
            rec["forward_k1_min_ms"], rec["forward_k4_min_ms"] = float(np.min(a)), float(np.min(b))
            rec["fused_backward_ms"], rec["fused_backward_min_ms"] = float(np.median(c)), float(np.min(c))
            rec["k1_vs_backward"] = rec["forward_k1_ms"] / rec["fused_backward_ms"]
            rec["k4_vs_k1"] = rec["forward_k4_ms"] / rec["forward_k1_ms"]
            # the same Jacobian in reverse mode: one backward per output row (steps * I controls, steps * 2 states),
            # only the gradients of the four weights asked for
            rows = S * (I + 2)

            def jacobian_by_backward():
                for _ in range(rows):
                    s.rollout_backward(S, *dev, nlt, sequences=seqs, states=states, grad_controls=gu, grad_states=gx,
                                       inputs=I, want=("Q", "R"), want_flags=False)
            jacobian_by_backward()
            d = [timed(jacobian_by_backward) for _ in range(max(3, args.reps // 5))]
            rec["jacobian_backward_calls"], rec["jacobian_by_backward_ms"] = rows, float(np.median(d))
            rec["jacobian_backward_vs_forward_k4"] = rec["jacobian_by_backward_ms"] / rec["forward_k4_ms"]
            s.rollout_forward(S, *dev, nlt, sequences=seqs, states=states, tangents=tan[4], inputs=I)
            rec["forward_flags"] = s.last_flags
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del dev, states, seqs, tan
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
