#!/usr/bin/env python3
"""Timing of the compact closed loop's backward pass (tpc_mpc_rollout_compact_exact_backward), fp64, DEVICE memory, in
one run on the same inputs and the same recorded forward:
  raw   rollout_compact_exact_backward with every output, against rollout_backward on the PRE-EXPANDED general-form
        arrays with every output (the parent's kernel; the expansion and the fold-back are not timed);
  step  a whole fitting step -- forward + backward of mean(states^2) with gradients to the four weights, v, delta_y and
        delta_phi -- through mpc_rollout_compact(backward="fused") against the default route (backward="expanded").
Also the routes' gradient differences (norm-wise, per leaf).  One JSON line per case; medians of --reps event-timed
calls after --warmup untimed ones.
usage: bench_rollout_compact_grad.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench_rollout_compact import CASES, timed
from trajectory_controller_amd import MpcSolver, compact_general_form, mpc_rollout_compact
from trajectory_controller_amd.autograd import _param_defaults
from trajectory_controller_amd.synth import compact_inputs

ALL = ("v", "delta_y", "delta_phi", "x0", "params", "params_rows", "kkt_residual")
LEAVES = ("weights", "v", "delta_y", "delta_phi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--max-rounds", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n, H, S in CASES:
        v, dy, dphi = (torch.from_numpy(a).cuda() for a in compact_inputs(H, n))
        pol = dict(tol=args.tol, max_rounds=args.max_rounds)
        rng = np.random.default_rng(3)
        with MpcSolver(horizon=H) as s:
            p = s.params
            gen = [t.contiguous() for t in compact_general_form(v, dy, dphi, *_param_defaults(p), H).values()]
            rec = dict(horizon=H, steps=S, n=n, **pol)
            c, x, q, st, first = s.rollout_compact_exact(S, v, dy, dphi, **pol)
            torch.cuda.synchronize()
            rec["forward_flags"] = s.last_flags
            rec["fell_back_share"] = float((first < S).double().mean())
            gc, gx = (torch.from_numpy(rng.standard_normal((2 * S, n))).cuda() for _ in range(2))

            # ---- the raw entries, every output, the same records and incoming gradient
            fused = lambda: s.rollout_compact_exact_backward(S, v, dy, dphi, sequences=q, states=x, grad_controls=gc,
                                                             grad_states=gx, want=ALL, want_flags=False)
            general = lambda: s.rollout_backward(S, *gen, None, sequences=q, states=x, grad_controls=gc,
                                                 grad_states=gx, inputs=2, want_flags=False)
            rec["raw_general_ms"], rec["raw_general_min_ms"] = timed(general, args.reps, args.warmup)
            rec["raw_fused_ms"], rec["raw_fused_min_ms"] = timed(fused, args.reps, args.warmup)
            rec["raw_general_over_fused"] = rec["raw_general_ms"] / rec["raw_fused_ms"]
            g, d = fused(), general()
            torch.cuda.synchronize()
            T, l = p.step_size, p.wheelbase
            Sm, D = d["A"][1] + d["B"][1], d["B"][2] - d["B"][3]
            ref = dict(v=T * Sm + (T / l) * D, delta_y=d["targets"][0::2].sum(dim=0), delta_phi=d["targets"][1::2].sum(dim=0),
                       x0=d["x0"])
            rel = lambda a, b: float(torch.linalg.norm(a - b) / torch.linalg.norm(b))
            rec["raw_difference"] = {k: rel(g[k], ref[k]) for k in ref}
            rec["raw_difference"]["weights"] = rel(g["params"][0:4], torch.stack(
                [d["Q"][0].sum(), d["Q"][1].sum(), d["R"][0].sum(), d["R"][1].sum()]))

            # ---- a whole fitting step through autograd
            w0 = [p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear]
            grads = {}

            def step(route):
                w = torch.tensor(w0, dtype=torch.float64, requires_grad=True)     # on the CPU: no device-to-host read
                tv, ty, tp = (t.detach().clone().requires_grad_() for t in (v, dy, dphi))
                _, states = mpc_rollout_compact(s, S, tv, ty, tp, weights=w, polish=(args.tol, args.max_rounds),
                                                backward=route)
                (states ** 2).mean().backward()
                grads[route] = [w.grad.to(v.device), tv.grad, ty.grad, tp.grad]

            for route in ("expanded", "fused"):
                rec[f"step_{route}_ms"], rec[f"step_{route}_min_ms"] = timed(lambda: step(route), args.reps, args.warmup)
            rec["step_expanded_over_fused"] = rec["step_expanded_ms"] / rec["step_fused_ms"]
            rec["forward_ms"], rec["forward_min_ms"] = timed(
                lambda: s.rollout_compact_exact(S, v, dy, dphi, want_status=False, **pol), args.reps, args.warmup)
            torch.cuda.synchronize()
            rec["step_difference"] = {k: rel(a, b) for k, a, b in zip(LEAVES, grads["fused"], grads["expanded"])}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
