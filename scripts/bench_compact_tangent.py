#!/usr/bin/env python3
"""Timing of the forward mode of the exact compact solve (solve_batch_compact_exact_forward:
tpc_mpc_solve_batch_compact_exact_forward) -- K columns of the per-instance Jacobian of (front, rear) with respect to
the shared parameters in one call -- beside the two ways the same Jacobian costs without it, on the same inputs in the
same run:
  - solve_batch_general_forward on the pre-expanded arrays and tangents with the same K (the expansion of the model
    and of the K directions timed separately: a fit pays it every step);
  - the two rows_backward calls (grad_front = 1, then grad_rear = 1) on a broadcast [10, n] tensor, which give all ten
    columns whatever K is.
K in {1, 4, 10} unit directions on the shared parameters ("params"; K = 4: the four weights), and K = 4 with
params_rows ("params_rows" [4, 10, n]).  fp64, DEVICE memory.  One JSON line per shape; medians (and the minimum and
maximum, for the spread) of --reps timed calls after --warmup untimed ones, measured with events on the launch stream.
usage: bench_compact_tangent.py [--reps 20] [--warmup 3] [--out profiles/r17_compact_tangent_timing.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.autograd import _param_defaults, compact_general_form
from trajectory_controller_amd.synth import compact_inputs

SHAPES = ((262144, 4), (262144, 10), (262144, 20), (16384, 40))   # (n, H)
KS = (1, 4, 10)


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
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def shared_rows(p, n, device):
    col = [p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear, p.step_size, p.wheelbase,
           p.lower[0], p.lower[1], p.upper[0], p.upper[1]]
    return torch.tensor(col, dtype=torch.float64, device=device)[:, None].expand(10, n).contiguous()


def expanded_tangents(p, v, tp):
    """solve_batch_general_forward's tangents of K directions tp [K, 10] on the shared parameters (tv = tdy = tdphi = 0)"""
    K, n = tp.shape[0], v.numel()
    T, l = p.step_size, p.wheelbase
    tvl = (T * v) / l
    tTv = tp[:, 4:5] * v[None]
    ttvl = (tTv - tvl[None] * tp[:, 5:6]) / l
    zero = torch.zeros_like(tTv)
    wide = lambda a: a[:, :, None].expand(K, a.shape[1], n).contiguous()
    return dict(A=torch.stack([zero, tTv, zero, zero], 1), B=torch.stack([zero, tTv, ttvl, -ttvl], 1),
                Q=wide(tp[:, 0:2]), R=wide(tp[:, 2:4]), lower=wide(tp[:, 6:8]), upper=wide(tp[:, 8:10]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n, H in SHAPES:
        v, dy, dphi = (torch.from_numpy(a).cuda() for a in compact_inputs(H, n))
        with MpcSolver(horizon=H) as s:
            p = s.params
            _, _, seq, st, _ = s.solve_batch_compact_exact(v, dy, dphi, want_sequence=True)
            rec = dict(horizon=H, n=n, excluded=int((st < 0).sum()), reps=args.reps)
            expand = lambda: [t.contiguous() for t in compact_general_form(v, dy, dphi, *_param_defaults(p), H).values()]
            ins = expand()
            rec["expand_model_ms"] = timed(expand, args.reps, args.warmup)
            eye = torch.eye(10, dtype=torch.float64, device=v.device)
            for K in KS:
                tp = eye[:K].contiguous()
                tan = {"params": tp}
                rec[f"compact_forward_K{K}_ms"] = timed(
                    lambda: s.solve_batch_compact_exact_forward(v, dy, dphi, seq, tan, status=st, want_flags=False),
                    args.reps, args.warmup)
                gt = expanded_tangents(p, v, tp)
                rec[f"expand_tangents_K{K}_ms"] = timed(lambda: expanded_tangents(p, v, tp), args.reps, args.warmup)
                rec[f"general_forward_K{K}_ms"] = timed(
                    lambda: s.solve_batch_general_forward(*ins, seq, gt, inputs=2, want_flags=False), args.reps, args.warmup)
                rec[f"general_over_compact_K{K}"] = (rec[f"general_forward_K{K}_ms"]["median"]
                                                     / rec[f"compact_forward_K{K}_ms"]["median"])
                tf, tr = s.solve_batch_compact_exact_forward(v, dy, dphi, seq, tan, status=st)
                tu = s.solve_batch_general_forward(*ins, seq, gt, inputs=2)
                ok = st >= 0
                rec[f"rel_diff_K{K}"] = float(max((tf[:, ok] - tu[:, 0][:, ok]).norm() / tu[:, 0][:, ok].norm(),
                                                  (tr[:, ok] - tu[:, 1][:, ok]).norm() / tu[:, 1][:, ok].norm()))
                del gt, tu
            # K = 4 with per-instance parameters
            rows = shared_rows(p, n, v.device)
            trows = eye[:4][:, :, None].expand(4, 10, n).contiguous()
            rec["compact_forward_rows_K4_ms"] = timed(
                lambda: s.solve_batch_compact_exact_forward(v, dy, dphi, seq, {"params_rows": trows}, status=st,
                                                            params_rows=rows, want_flags=False), args.reps, args.warmup)
            # the same Jacobian in reverse mode: two rows_backward calls, ten rows each
            one = torch.ones_like(v)

            def two_backwards():
                for gf, gr in ((one, None), (None, one)):
                    s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, status=st, want=("params_rows",),
                                                         params_rows=rows, want_flags=False)
            rec["two_rows_backward_ms"] = timed(two_backwards, args.reps, args.warmup)
            for K in KS:
                rec[f"two_backwards_over_compact_K{K}"] = (rec["two_rows_backward_ms"]["median"]
                                                           / rec[f"compact_forward_K{K}_ms"]["median"])
            # ... and they are the same numbers
            jac = [s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, status=st, want=("params_rows",),
                                                        params_rows=rows)["params_rows"]
                   for gf, gr in ((one, None), (None, one))]
            tf, tr = s.solve_batch_compact_exact_forward(v, dy, dphi, seq, {"params": eye}, status=st)
            rec["rel_diff_reverse"] = float(max((tf - jac[0]).norm() / jac[0].norm(), (tr - jac[1]).norm() / jac[1].norm()))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
