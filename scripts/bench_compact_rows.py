#!/usr/bin/env python3
"""Timing of the fitting step with PER-INSTANCE parameters through the exact compact route (mpc_compact_exact with
[.., n] parameters: forward tpc_mpc_solve_batch_compact_exact_rows, backward
tpc_mpc_solve_batch_compact_exact_rows_backward) beside the general-form route mpc_compact(..., polish=True), which is
the yardstick, on the same inputs in the same run: forward plus backward of a mean-square loss on (front, rear) against
logged steering, with gradients to the per-instance weights [4, n] and to v, dy and dphi.  Beside them the shared
mpc_compact_exact step with the default model (what constant rows would hold), to show what reading rows costs over
kernel arguments.  Two recipes of per-instance parameters: "weights" (the four weights drawn per instance) and "all"
(weights, step_size, wheelbase and both bounds), as tests/model/compact_rows_common.py draws them.  fp64, DEVICE memory.
One JSON line per shape and recipe; medians of --reps timed iterations after --warmup untimed ones, measured with
events on the launch stream.
usage: bench_compact_rows.py [--reps 20] [--warmup 3] [--out profiles/r15_compact_rows_timing.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trajectory_controller_amd import MpcSolver, mpc_compact, mpc_compact_exact
from trajectory_controller_amd.synth import compact_inputs

SHAPES = ((262144, 4), (262144, 10), (262144, 20), (16384, 40))   # (n, H)
AMAX = 22.0 * np.pi / 180.0


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


def recipe(name, H, n):
    """the per-instance parameters of a recipe as keyword arguments of both routes (CUDA tensors); the draws of
    tests/model/compact_rows_common.recipe_rows"""
    rng = np.random.default_rng(1000 + H)
    w = np.array([20, 7, 0.0005, 10])[:, None] * np.exp(0.5 * rng.standard_normal((4, n)))
    T = rng.uniform(0.05, 0.15, n)
    l = rng.uniform(0.15, 0.35, n)
    lo = -AMAX * rng.uniform(0.5, 1, (2, n))
    hi = AMAX * rng.uniform(0.5, 1, (2, n))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = dict(step_size=up(T), wheelbase=up(l), lower=up(lo), upper=up(hi)) if name == "all" else {}
    return up(w).requires_grad_(), kw


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
            w0 = torch.tensor([p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear],
                              dtype=torch.float64, device="cuda", requires_grad=True)

            def step(route, w, kw):
                for t in (v, dy, dphi, w):
                    t.grad = None
                if route == "general":
                    dflt = dict(step_size=p.step_size, wheelbase=p.wheelbase, lower=tuple(p.lower), upper=tuple(p.upper))
                    front, rear = mpc_compact(s, v, dy, dphi, w, polish=True, **{**dflt, **kw})
                else:
                    front, rear = mpc_compact_exact(s, v, dy, dphi, weights=w, **kw)
                loss = ((front - logged[0]) ** 2 + (rear - logged[1]) ** 2).mean()
                loss.backward()
                return loss

            shared_ms, shared_min = timed(lambda: step("exact", w0, {}), args.reps, args.warmup)
            for name in ("weights", "all"):
                w, kw = recipe(name, H, n)
                rec = dict(horizon=H, n=n, recipe=name)
                grads = {}
                rec["general_polish_step_ms"], rec["general_polish_step_min_ms"] = timed(
                    lambda: step("general", w, kw), args.reps, args.warmup)
                grads["general"] = [t.grad.clone() for t in (v, dy, dphi, w)]
                rec["exact_rows_step_ms"], rec["exact_rows_step_min_ms"] = timed(
                    lambda: step("exact", w, kw), args.reps, args.warmup)
                grads["exact"] = [t.grad.clone() for t in (v, dy, dphi, w)]
                rec["exact_shared_step_ms"], rec["exact_shared_step_min_ms"] = shared_ms, shared_min
                rec["speedup_of_the_step"] = rec["general_polish_step_ms"] / rec["exact_rows_step_ms"]
                rec["rows_over_shared"] = rec["exact_rows_step_ms"] / shared_ms
                # who fell back, who is left, and the raw entries alone
                rows = torch.empty(10, n, dtype=torch.float64, device="cuda")
                rows[0:4] = w.detach()
                dflt = [p.step_size, p.wheelbase, p.lower[0], p.lower[1], p.upper[0], p.upper[1]]
                rows[4:10] = torch.tensor(dflt, dtype=torch.float64, device="cuda")[:, None]
                if kw:
                    rows[4], rows[5], rows[6:8], rows[8:10] = kw["step_size"], kw["wheelbase"], kw["lower"], kw["upper"]
                vd, yd, pd = v.detach(), dy.detach(), dphi.detach()
                _, _, seq, st, fell = s.solve_batch_compact_exact(vd, yd, pd, want_sequence=True, params_rows=rows)
                rec["flags_solve"] = s.last_flags
                rec["fell_back"] = int(fell.sum())
                rec["left_unverified"] = int((st < 0).sum())
                rec["phase1_ms"], _ = timed(lambda: s.solve_batch_compact_exact(
                    vd, yd, pd, fallback="none", want_status=False, params_rows=rows), args.reps, args.warmup)
                rec["forward_ms"], _ = timed(lambda: s.solve_batch_compact_exact(
                    vd, yd, pd, want_sequence=True, params_rows=rows), args.reps, args.warmup)
                rec["backward_rows_ms"], _ = timed(lambda: s.solve_batch_compact_exact_backward(
                    vd, yd, pd, seq, logged[0], logged[1], status=st, want=("v", "delta_y", "delta_phi", "params_rows"),
                    want_flags=False, params_rows=rows), args.reps, args.warmup)
                # the two routes' gradients on the instances neither left unverified (the general route's own
                # unverified instances carry its solver's eps-0.01 point and are not comparable)
                keep = st >= 0
                for gname, a, b in zip(("v", "delta_y", "delta_phi", "weights"), grads["exact"], grads["general"]):
                    a, b = a[..., keep], b[..., keep]
                    rec[f"median_abs_diff_d{gname}"] = float((a - b).abs().median())
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
