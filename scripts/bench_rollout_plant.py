#!/usr/bin/env python3
"""Timing of the closed loops against a separate plant, fp64, two inputs, DEVICE memory, on the
shapes of profiles/r11_rollout_tangent_timing.jsonl: rollout_newton, rollout_backward and rollout_forward (K = 1 and 4)
-- the parent entries -- and the same calls through the plant entries, once with the plant set to copies of the
controller's model and once with the mismatched plant and a disturbance.  The yardstick of every plant call is its
parent in the same run: everything is interleaved, medians of --reps event-timed calls after --warmup untimed ones,
and the parent's own spread ((max - min) / median of its repeats) is reported beside every ratio.
usage: bench_rollout_plant.py [--reps 20] [--warmup 3] [--out profiles/r12_rollout_plant_timing.jsonl]"""
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
SCALE = 0.05                                                    # the tests' mismatch (tests/test_rollout_plant_host.py)


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
        nlt = (dev[8][2 * (H - 1):2 * H].repeat(S, 1) + 0.01 * rnd(2 * S, n)).contiguous()
        gu, gx = rnd(S * I, n), rnd(2 * S, n)
        plants = {"copy": (tuple(a.clone() for a in dev[:3]), None),
                  "mismatch": ((dev[0] * (1 + SCALE * rnd(4, n)), dev[1] * (1 + SCALE * rnd(2 * I, n)),
                                dev[2] + SCALE * rnd(2, n)), 0.1 * SCALE * rnd(2 * S, n))}
        with MpcSolver(horizon=H) as s:
            rec = dict(inputs=I, horizon=H, steps=S, n=n)
            calls = {}
            for tag, (plant, dist) in [("parent", (None, None))] + list(plants.items()):
                kw = {} if plant is None else dict(plant=plant, disturbance=dist)
                _, states, seqs, *_ = s.rollout_newton(S, *dev, nlt, inputs=I, want_status=False, **kw)
                bkw = {} if plant is None else dict(plant=plant)
                calls[tag, "newton"] = lambda kw=kw: s.rollout_newton(S, *dev, nlt, inputs=I, want_status=False, **kw)
                calls[tag, "backward"] = lambda st=states, sq=seqs, kw=bkw: s.rollout_backward(
                    S, *dev, nlt, sequences=sq, states=st, grad_controls=gu, grad_states=gx, inputs=I, want_flags=False,
                    **kw)
                for K in (1, 4):
                    tan = {"Q": rnd(K, 2, n), "R": rnd(K, I, n)}
                    if plant is not None:
                        tan.update(Ap=rnd(K, 4, n), disturbance=rnd(K, 2 * S, n))
                    calls[tag, f"forward_k{K}"] = lambda st=states, sq=seqs, kw=bkw, tan=tan: s.rollout_forward(
                        S, *dev, nlt, sequences=sq, states=st, tangents=tan, inputs=I, want_flags=False, **kw)
            for _ in range(args.warmup):
                for fn in calls.values():
                    fn()
            t = {k: [] for k in calls}
            for _ in range(args.reps):   # interleaved, so drift hits all alike
                for k, fn in calls.items():
                    t[k].append(timed(fn))
            for what in ("newton", "backward", "forward_k1", "forward_k4"):
                base = t["parent", what]
                rec[f"{what}_parent_ms"] = float(np.median(base))
                rec[f"{what}_parent_spread"] = float((np.max(base) - np.min(base)) / np.median(base))
                for tag in plants:
                    rec[f"{what}_{tag}_ms"] = float(np.median(t[tag, what]))
                    rec[f"{what}_{tag}_vs_parent"] = rec[f"{what}_{tag}_ms"] / rec[f"{what}_parent_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del dev, calls, plants
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
