#!/usr/bin/env python3
"""Timing of the weight-fitting step through the exact compact route (mpc_compact_exact: forward
tpc_mpc_solve_batch_compact_exact, backward tpc_mpc_solve_batch_compact_exact_backward) beside the general-form route
mpc_compact(..., polish=True) on the same inputs in the same run: forward plus backward of a mean-square loss on
(front, rear) against logged steering, with gradients to the four weights and to v, dy and dphi.  Also the raw backward
entry alone against solve_batch_general_backward on the expanded arrays (every output of each).  fp64, DEVICE memory.
One JSON line per shape; medians of --reps timed iterations after --warmup untimed ones, measured with events on the
launch stream.
usage: bench_compact_grad.py [--reps 20] [--warmup 3] [--out profiles/r14_compact_grad_timing.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trajectory_controller_amd import MpcSolver, compact_general_form, mpc_compact, mpc_compact_exact
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n, H in SHAPES:
        v, dy, dphi = (torch.from_numpy(a).cuda().requires_grad_() for a in compact_inputs(H, n))
        rng = np.random.default_rng(H)
        logged = [torch.from_numpy(0.1 * rng.standard_normal(n)).cuda() for _ in range(2)]
        with MpcSolver(horizon=H) as s:
            p = s.params
            w0 = [p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear]
            rec = dict(horizon=H, n=n)
            grads = {}
            for where in ("cuda", "cpu"):
                w = torch.tensor(w0, dtype=torch.float64, device=where, requires_grad=True)

                def step(route, w=w):
                    for t in (v, dy, dphi, w):
                        t.grad = None
                    if route == "exact":
                        front, rear = mpc_compact_exact(s, v, dy, dphi, weights=w)
                    else:
                        front, rear = mpc_compact(s, v, dy, dphi, w.to(v.device), polish=True)
                    loss = ((front - logged[0]) ** 2 + (rear - logged[1]) ** 2).mean()
                    loss.backward()
                    return loss
                if where == "cuda":
                    rec["general_polish_step_ms"], rec["general_polish_step_min_ms"] = timed(
                        lambda: step("general"), args.reps, args.warmup)
                    grads["general"] = [t.grad.clone() for t in (v, dy, dphi, w)]
                rec[f"exact_step_weights_on_{where}_ms"], rec[f"exact_step_weights_on_{where}_min_ms"] = timed(
                    lambda: step("exact"), args.reps, args.warmup)
                if where == "cuda":
                    grads["exact"] = [t.grad.clone() for t in (v, dy, dphi, w)]
            rec["speedup_of_the_step"] = rec["general_polish_step_ms"] / rec["exact_step_weights_on_cuda_ms"]
            for name, a, b in zip(("v", "delta_y", "delta_phi", "weights"), grads["exact"], grads["general"]):
                rec[f"rel_diff_d{name}"] = float((a - b).norm() / b.norm())

            # the raw backward entries alone, every output of each
            vd, yd, pd = v.detach(), dy.detach(), dphi.detach()
            front, rear, seq, st, _ = s.solve_batch_compact_exact(vd, yd, pd, want_sequence=True)
            gf, gr = [torch.from_numpy(rng.standard_normal(n)).cuda() for _ in range(2)]
            want = ("v", "delta_y", "delta_phi", "params", "params_rows", "kkt_residual")
            rec["compact_backward_ms"], _ = timed(
                lambda: s.solve_batch_compact_exact_backward(vd, yd, pd, seq, gf, gr, status=st, want_flags=False),
                args.reps, args.warmup)
            rec["compact_backward_all_outputs_ms"], _ = timed(
                lambda: s.solve_batch_compact_exact_backward(vd, yd, pd, seq, gf, gr, status=st, want=want,
                                                             want_flags=False), args.reps, args.warmup)
            ins = [t.contiguous() for t in compact_general_form(vd, yd, pd, *_param_defaults(p), H).values()]
            g = torch.zeros_like(seq)
            g[0], g[1] = gf, gr
            rec["general_backward_ms"], _ = timed(
                lambda: s.solve_batch_general_backward(*ins, seq, g, inputs=2, want_flags=False), args.reps, args.warmup)
            rec["speedup_of_the_backward"] = rec["general_backward_ms"] / rec["compact_backward_ms"]
            rec["excluded"] = int((st < 0).sum())
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
