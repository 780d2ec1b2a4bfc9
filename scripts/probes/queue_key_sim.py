#!/usr/bin/env python3
"""Probe (CPU): tests/extended/stop_depth_sim.py's lockstep simulation on numpy arrays, for the queue keys of the fp64 N = 20
kernels -- lambda (a function of the speed), the committed table (csrc/mpc_queue_key_table.h) and the true count: 16
wavefronts x 64 lanes fed longest-first from every 16th instance of the headline batch; per key the fraction of wave
iterations in which all 64 lanes are decided after the check steps, the instructions of 530 the checks save, the wave
iterations of the busiest wavefront and the lane utilisation.

    python scripts/probes/queue_key_sim.py [path of a built tests/extended/stop_depth_stats]

Without the argument the tool is compiled (g++) into a temporary directory.
"""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_queue_key_table as qk
from trajectory_controller_amd.synth import compact_inputs

H, N, EVERY, WAVES = 20, 262144, 16, 16
v, dy, dphi = compact_inputs(H, N)
idx = np.arange(0, N, EVERY)
am = 22 * math.pi / 180
with tempfile.TemporaryDirectory() as tmp:
    tool = sys.argv[1] if len(sys.argv) > 1 else os.path.join(tmp, "stop_depth_stats")
    if len(sys.argv) <= 1:
        subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-std=c++17", "-o", tool,
                               os.path.join(ROOT, "tests", "extended", "stop_depth_stats.cpp")])
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.concatenate([v[idx], dy[idx], dphi[idx]]).tofile(fin)
    subprocess.check_call([tool, fin, str(len(idx)), fout, "20", "7", "0.0005", "10", "0.1", "0.21", repr(-am), repr(am)])
    b = open(fout, "rb").read()
pos, starts, lengths = 0, [], []
chunks = []
while pos < len(b):
    cnt = int(np.frombuffer(b, dtype=np.uint32, count=1, offset=pos)[0]); pos += 8
    chunks.append(np.frombuffer(b, dtype=np.uint8, count=cnt, offset=pos)); pos += cnt
    lengths.append(cnt)
lengths = np.array(lengths)
starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
flat = np.concatenate(chunks)


def simulate(queue):
    L = WAVES * 64
    cur = np.array(queue[:L]); p = np.zeros(L, dtype=np.int64); live = np.ones(L, dtype=bool)
    qi = L
    wh = np.zeros((WAVES, H + 2), dtype=np.int64)
    busy = 0
    while live.any():
        d = np.where(live, flat[np.minimum(starts[cur] + p, len(flat) - 1)], 0).reshape(WAVES, 64)
        md = d.max(axis=1)
        wh[np.arange(WAVES)[md > 0], md[md > 0]] += 1
        busy += int(live.sum())
        p += live
        for l in np.flatnonzero(live & (p >= lengths[cur])):
            if qi < len(queue):
                cur[l], p[l] = queue[qi], 0; qi += 1
            else:
                live[l] = False
    per_wave = wh.sum(axis=1)
    c = np.cumsum(wh.sum(axis=0)) / wh.sum()
    return c, int(per_wave.max()), busy / (64.0 * per_wave.sum())


table, _ = qk.load_header()
keys = (("lambda (speed)", v[idx]), ("table, trilinear", qk.predict(table, v[idx], dy[idx], dphi[idx]).astype(np.float64)), ("true count", lengths.astype(np.float64)))
for name, key in keys:
    q = [int(i) for i in np.argsort(-key, kind="stable") if lengths[i]]
    c, longest, util = simulate(q)
    line = f"{name:18s} corr {np.corrcoef(key, lengths)[0, 1]:.3f}  decided after 2 / 5: {c[2]:.3f} / {c[5]:.3f}  after 3 / 8: {c[3]:.3f} / {c[8]:.3f}  wave iterations (max) {longest}  utilisation {util:.3f} "
    for ks in ((2, 5), (3, 8)):
        saved, prev, cost, reach = 0.0, 0.0, 0.0, 1.0
        for k in ks:
            saved += (c[k] - prev) * 6 * (H - k); cost += 3 * reach; reach = 1 - c[k]; prev = c[k]
        line += f" checks {ks}: {saved - cost:.1f} of 530 saved;"
    print(line)
