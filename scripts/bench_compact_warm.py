#!/usr/bin/env python3
"""Timing of the warm-started exact compact solve (tpc_mpc_solve_batch_compact_exact_from,
MpcSolver.solve_batch_compact_exact(start=...), mpc_compact_exact(warm=...)) beside the cold entry, which is the
yardstick, on the same inputs in the same run.  A chain of --steps optimiser steps whose four weights lie 1 % apart
(+, -, +, - per step); at every step the warm calls start from the sequence the warm chain's previous step returned
under fallback="solve" (step 1 has none: its warm calls get a start of zeros, which is the cold start on the warm
kernels).  Per step and call kind the median of --reps event-timed calls, the kinds interleaved inside every repetition;
the cold entry is timed twice per repetition (slots a and b), so that the distance between its own two medians is
known.  Recorded per step: phase 1 alone (fallback="none", no status: asynchronous) cold a / b and warm; the forward with
fallback="solve" cold a / b and warm, with who fell back, who is left and the mean rounds of the instances phase 1
verified; the whole fitting step (forward plus backward of a mean-square loss against logged steering) through
mpc_compact_exact without and with warm=.  Models: the shared default model and the two rows recipes of
tests/model/compact_rows_common.py.  After each chain one summary line: medians over steps 2.., and whether the warm
forward was slower than the cold one by more than the cold entry's own spread.  fp64, DEVICE memory, AUTO, tol 1e-9, 16
rounds.
usage: bench_compact_warm.py [--reps 20] [--warmup 2] [--steps 10] [--out profiles/r16_compact_warm_timing.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trajectory_controller_amd import CompactWarmStart, MpcSolver, mpc_compact_exact
from trajectory_controller_amd.synth import compact_inputs

SHAPES = ((262144, 4), (262144, 10), (262144, 20), (16384, 40))   # (n, H)
MODELS = ("shared", "weights", "all")
AMAX = 22.0 * np.pi / 180.0
SIGNS = np.array([1.0, -1.0, 1.0, -1.0])
TOL, ROUNDS = 1e-9, 16


def interleaved(fns, reps, warmup):
    """{name: median ms} of the calls in fns, all of them run in turn inside every repetition"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: float(np.median(x)) for k, x in ms.items()}


def rows_of(name, H, n, p):
    """params_rows [10, n] of a recipe (the draws of tests/model/compact_rows_common.recipe_rows; "shared": the
    solver's own ten values in every column), on the host"""
    rng = np.random.default_rng(1000 + H)
    col = [p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear, p.step_size, p.wheelbase,
           p.lower[0], p.lower[1], p.upper[0], p.upper[1]]
    rows = np.tile(np.array(col)[:, None], (1, n))
    if name == "shared":
        return rows
    rows[0:4] = np.array([20, 7, 0.0005, 10])[:, None] * np.exp(0.5 * rng.standard_normal((4, n)))
    T = rng.uniform(0.05, 0.15, n)
    l = rng.uniform(0.15, 0.35, n)
    lo = -AMAX * rng.uniform(0.5, 1, (2, n))
    hi = AMAX * rng.uniform(0.5, 1, (2, n))
    if name == "all":
        rows[4], rows[5], rows[6:8], rows[8:10] = T, l, lo, hi
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for n, H in SHAPES:
        v, dy, dphi = (up(a) for a in compact_inputs(H, n))
        rng = np.random.default_rng(H)
        logged = [up(0.1 * rng.standard_normal(n)) for _ in range(2)]
        for model in MODELS:
            with MpcSolver(horizon=H) as s:
                p = s.params
                base = rows_of(model, H, n, p)
                per = model != "shared"
                seq_prev = torch.zeros(2 * H, n, dtype=torch.float64, device="cuda")
                holder = CompactWarmStart()
                recs = []
                for step in range(args.steps):
                    scale = (1.0 + 0.01 * SIGNS) ** step
                    if per:
                        rows = base.copy()
                        rows[0:4] *= scale[:, None]
                        trows = up(rows)
                        fw = dict(params_rows=trows)
                        w = trows[0:4].clone().requires_grad_()
                        gkw = {} if model == "weights" else dict(step_size=trows[4], wheelbase=trows[5],
                                                                 lower=trows[6:8], upper=trows[8:10])
                    else:
                        wv = base[0:4, 0] * scale
                        fw = dict(weight_y=wv[0], weight_phi=wv[1], weight_steering_front=wv[2],
                                  weight_steering_rear=wv[3])
                        w = torch.tensor(wv, dtype=torch.float64, requires_grad=True)        # on the CPU: no read-back
                        gkw = {}
                    start = seq_prev

                    def phase1(st):
                        s.solve_batch_compact_exact(v, dy, dphi, tol=TOL, max_rounds=ROUNDS, fallback="none",
                                                    want_status=False, start=st, **fw)

                    def forward(st):
                        return s.solve_batch_compact_exact(v, dy, dphi, tol=TOL, max_rounds=ROUNDS, fallback="solve",
                                                           want_sequence=True, start=st, **fw)

                    def fit(warm):
                        w.grad = None
                        if warm is not None:
                            warm.sequence = start            # every repetition starts where the chain stands
                        front, rear = mpc_compact_exact(s, v, dy, dphi, weights=w, tol=TOL, max_rounds=ROUNDS, warm=warm,
                                                        **gkw)
                        ((front - logged[0]) ** 2 + (rear - logged[1]) ** 2).mean().backward()

                    ms = interleaved({
                        "phase1_cold_a": lambda: phase1(None), "phase1_warm": lambda: phase1(start),
                        "phase1_cold_b": lambda: phase1(None),
                        "forward_cold_a": lambda: forward(None), "forward_warm": lambda: forward(start),
                        "forward_cold_b": lambda: forward(None),
                        "step_cold_a": lambda: fit(None), "step_warm": lambda: fit(holder),
                        "step_cold_b": lambda: fit(None)}, args.reps, args.warmup)
                    rec = dict(horizon=H, n=n, model=model, step=step + 1, has_start=step > 0)
                    rec.update({f"{k}_ms": x for k, x in ms.items()})
                    for name, st in (("cold", None), ("warm", start)):
                        _, _, seq, status, fell = forward(st)
                        torch.cuda.synchronize()
                        p1 = (status >= 0) & (fell == 0)
                        rec[f"{name}_fell_back"] = int(fell.sum())
                        rec[f"{name}_left_unverified"] = int((status < 0).sum())
                        rec[f"{name}_phase1_mean_rounds"] = float(status[p1].double().mean())
                        rec[f"{name}_flags"] = s.last_flags
                    seq_prev = seq                                  # the warm chain's sequence_out
                    emit(rec)
                    recs.append(rec)
                tail = recs[1:] or recs
                med = lambda k: float(np.median([r[k] for r in tail]))
                summary = dict(horizon=H, n=n, model=model, summary=True, steps=len(tail))
                for kind in ("phase1", "forward", "step"):
                    a, b, wm = med(f"{kind}_cold_a_ms"), med(f"{kind}_cold_b_ms"), med(f"{kind}_warm_ms")
                    # the cold entry's own spread: the largest distance between its two medians at one step
                    spread = max(abs(r[f"{kind}_cold_a_ms"] - r[f"{kind}_cold_b_ms"]) for r in tail)
                    cold = 0.5 * (a + b)
                    summary.update({f"{kind}_cold_ms": cold, f"{kind}_warm_ms": wm, f"{kind}_cold_spread_ms": spread,
                                    f"{kind}_warm_over_cold": wm / cold,
                                    f"{kind}_warm_slower_beyond_spread": bool(any(
                                        r[f"{kind}_warm_ms"] > max(r[f"{kind}_cold_a_ms"], r[f"{kind}_cold_b_ms"]) + spread
                                        for r in tail))})
                for k in ("cold_fell_back", "warm_fell_back", "cold_phase1_mean_rounds", "warm_phase1_mean_rounds"):
                    summary[k] = med(k)
                emit(summary)


if __name__ == "__main__":
    main()
