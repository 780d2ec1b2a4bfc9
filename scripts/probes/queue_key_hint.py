#!/usr/bin/env python3
"""Probe (GPU): what ordering the N = 20 work queue by a table-predicted iteration count buys, BEFORE any kernel code --
the prediction (csrc/mpc_queue_key_table.h, trilinear: scripts/gen_queue_key_table.py predict) is computed on the host for
the headline batch and passed through the experimental work hint, which replaces float(lambda) as the key.

    python scripts/probes/queue_key_hint.py [rounds] [n]

Per round, interleaved on one box: a solve without the hint, one with the table hint, and (last rounds) one with the true
counts as the hint; kernel times (cd, pg) and lane statistics of each.  Record: profiles/r07_queue_key_hint.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch
import gen_queue_key_table as qk
from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import compact_inputs

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
H = 20
v, dy, dphi = compact_inputs(H, n)
table, dims = qk.load_header()
pred = qk.predict(table, v, dy, dphi)
hint_tab = torch.from_numpy(np.maximum(np.rint(pred.astype(np.float64) * 16.0), 1).astype(np.int32)).cuda()   # (x16: only the order counts)
tv, ty, tp = (torch.from_numpy(a).cuda() for a in (v, dy, dphi))
s = MpcSolver(horizon=H, algo="auto")
s.set_profiling(True)
f0, r0, it0 = s.solve_batch_compact(tv, ty, tp, want_iters=True)
torch.cuda.synchronize()
cnt = it0.cpu().numpy().astype(np.float64)


def ranks(a):
    r = np.empty(len(a))
    r[np.argsort(a, kind="stable")] = np.arange(len(a))
    return r


print(f"table {table.shape}, {dims['Samples']} samples per node; n = {n}, N = {H}, fp64, AUTO")
print(f"Spearman with the count: v {np.corrcoef(ranks(v), ranks(cnt))[0, 1]:.4f}  table {np.corrcoef(ranks(pred), ranks(cnt))[0, 1]:.4f};"
      f"  Pearson of log: table {np.corrcoef(np.log(pred), np.log(np.maximum(cnt, 1)))[0, 1]:.4f}")
hint_true = it0.to(torch.int32).clamp(min=1).contiguous()
res = {"lambda": [], "table": [], "true": []}
for rnd in range(rounds):
    for name, hint in (("lambda", None), ("table", hint_tab), ("true", hint_true)):
        if name == "true" and rnd < rounds - 3:
            continue
        s.set_work_hint(hint)
        f, r, it = s.solve_batch_compact(tv, ty, tp, want_iters=True)
        k1, k2, algo = s.last_kernel_times()
        wi, rb = s.last_lane_stats()
        same = bool(torch.equal(f, f0) and torch.equal(r, r0) and torch.equal(it, it0))
        res[name].append((k1, k2, wi))
        print(f"round {rnd} {name:6s}: cd {k1:.4f} ms  pg {k2:.4f} ms  wave_iterations {wi}  refills {rb}  algo {algo}  bits equal {same}")
for name, rs in res.items():
    if rs:
        a = np.array(rs)
        print(f"{name:6s}: pg min {a[:, 1].min():.4f} median {np.median(a[:, 1]):.4f} max {a[:, 1].max():.4f} ms;  cd median {np.median(a[:, 0]):.4f} ms;"
              f"  wave_iterations median {np.median(a[:, 2]):.0f}")
