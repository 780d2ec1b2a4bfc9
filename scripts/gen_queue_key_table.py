#!/usr/bin/env python3
"""Generator of csrc/mpc_queue_key_table.h (`make regen`): the table behind the queue key of the fp64 N = 20
coordinate-descent kernel -- log2 of dlib's iteration count over (log v, dy, dphi), looked up trilinearly
(csrc/mpc_queue_key.h) where the kernel used float(lambda), a function of the speed alone.

    python3 scripts/gen_queue_key_table.py [NV NY NP [SAMPLES]] > trajectory_controller_amd/csrc/mpc_queue_key_table.h

The box is the one the reference's code gives its controller (v in [0.1, 4] m/s after the velocity lookup, y_soll in
+-0.5 m, phi_soll in +-0.6 rad); nodes are uniform in log v, dy and dphi and include the box's faces.  The count is jagged in
its inputs (single instances take 2.4-3.6 times what their neighbours do), so a node is not ONE solve: it is the mean of
log2(count) over SAMPLES seeded instances drawn uniformly from the node's cell (half a spacing to each side, cut at the
box).  Sampling is stratified, so no cell is empty; should one ever be (SAMPLES = 0 for a cell in a variant of this script),
it takes the mean of its speed slice (fill_empty).  Counts come from the project's own checker, oracle/mpc_oracle.c, with
the parameters recorded in the header: a handle with any other parameter set keeps lambda (tpc_mpc_api.cpp).
Above the box the lookup continues the speed axis with its last cell's slope up to V_CAP (the count keeps growing there);
the header records V_CAP and the nodes that takes.
The sample stream is splitmix64 with a seed of its own -- not the synthetic bench stream's (synth.compact_inputs).
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from trajectory_controller_amd.synth import splitmix64_uniform   # noqa: E402

H = 20
SHAPE = (32, 12, 12)
SAMPLES = 48
SEED = 0x7AB1E000 + H
V_LO, V_HI = 0.1, 4.0
DY_MAX, DPHI_MAX = 0.5, 0.6
V_CAP = 4.0 * V_HI    # above the box the lookup continues the speed axis with its last cell's slope, up to here
WEIGHTS = (20.0, 7.0, 0.0005, 10.0)
STEP, WHEELBASE = 0.1, 0.21
ALPHA_MAX = 22.0 * math.pi / 180.0
EPS, MAX_ITER, SMO_ITERS = 0.01, 10000, 50


def axes(shape=SHAPE):
    """(lo, hi) of the three coordinates (log v, dy, dphi) and the node spacing of each"""
    lo = np.array([math.log(V_LO), -DY_MAX, -DPHI_MAX])
    hi = np.array([math.log(V_HI), DY_MAX, DPHI_MAX])
    return lo, hi, (hi - lo) / (np.array(shape) - 1)


def axis_consts(shape=SHAPE):
    """what the lookup works with, in float32: each coordinate's lower face and nodes per unit"""
    lo, hi, _ = axes(shape)
    return lo.astype(np.float32), ((np.array(shape) - 1) / (hi - lo)).astype(np.float32)


def cell_samples(cells, shape=SHAPE, samples=SAMPLES):
    """(v, dy, dphi), each [len(cells), samples]: the seeded instances of the cells (flat node indices)"""
    cells = np.asarray(cells, dtype=np.int64)
    lo, hi, d = axes(shape)
    node = np.stack(np.unravel_index(cells, shape), axis=1)                      # [c, 3]
    c_lo = np.maximum(lo + (node - 0.5) * d, lo)
    c_hi = np.minimum(lo + (node + 0.5) * d, hi)
    u = np.stack([splitmix64_uniform(SEED, 3 * samples, offset=3 * samples * int(c)).reshape(samples, 3) for c in cells])
    p = c_lo[:, None, :] + u * (c_hi - c_lo)[:, None, :]                         # [c, samples, 3]
    return np.exp(p[..., 0]), p[..., 1], p[..., 2]


def cell_values(cells, shape=SHAPE, samples=SAMPLES, nthreads=None):
    """mean log2(iteration count) of the cells' samples, fp64 (NaN for a cell without samples)"""
    from oracle.bindings import Oracle
    v, dy, dphi = cell_samples(cells, shape, samples)
    if v.size == 0:
        return np.full(len(cells), np.nan)
    nthreads = nthreads or min(16, os.cpu_count() or 1)
    _, _, it = Oracle().solve_compact(H, v.ravel(), dy.ravel(), dphi.ravel(), weights=WEIGHTS, T=STEP, l=WHEELBASE,
                                      lo=(-ALPHA_MAX, -ALPHA_MAX), hi=(ALPHA_MAX, ALPHA_MAX), eps=EPS, max_iter=MAX_ITER,
                                      smo_iters=SMO_ITERS, nthreads=nthreads)
    return np.log2(np.maximum(it, 1).astype(np.float64)).reshape(v.shape).mean(axis=1)


def fill_empty(table):
    """cells without samples (NaN) take the mean of their speed slice"""
    for s in table:
        if np.isnan(s).any():
            s[np.isnan(s)] = np.nanmean(s)
    return table


def make_table(shape=SHAPE, samples=SAMPLES):
    n = int(np.prod(shape))
    return fill_empty(cell_values(np.arange(n), shape, samples).reshape(shape)).astype(np.float32)


def v_beyond(shape=SHAPE):
    """whole nodes of the speed axis past its upper face that reach V_CAP"""
    return int(math.ceil(math.log(V_CAP / V_HI) / axes(shape)[2][0]))


def predict(table, v, dy, dphi):
    """numpy restatement of csrc/mpc_queue_key.h: the predicted iteration count (float32), targets clamped into
    the box and the speed into [V_LO, V_CAP] (NaN goes to the lower face), trilinear in float32; above V_HI the last
    cell of the speed axis is continued (a weight above 1)"""
    f32 = np.float32
    def clamp(x, a, b):   # (fp64, before anything is narrowed or turned into an index; NaN fails `>` and lands on a)
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            x = np.where(x > a, x, a)
            return np.where(x < b, x, b)
    c = [np.log(clamp(v, V_LO, V_CAP).astype(f32)), clamp(dy, -DY_MAX, DY_MAX).astype(f32), clamp(dphi, -DPHI_MAX, DPHI_MAX).astype(f32)]
    idx, frac = [], []
    lo32, scale32 = axis_consts(table.shape)
    for a in range(3):
        n = table.shape[a]
        top = n - 1 + (v_beyond(table.shape) if a == 0 else 0)
        with np.errstate(invalid="ignore"):
            f = (c[a] - lo32[a]) * scale32[a]
            f = np.where(f > 0, f, f32(0))
            f = np.where(f < top, f, f32(top))
        i = np.minimum(f.astype(np.int32), n - 2)
        idx.append(i)
        frac.append((f - i.astype(f32)).astype(f32))
    (i, j, k), (a, b, g) = idx, frac
    t = table.astype(f32)

    def lerp(p, q, w):
        return (p + w * (q - p)).astype(f32)
    c00, c01 = lerp(t[i, j, k], t[i, j, k + 1], g), lerp(t[i, j + 1, k], t[i, j + 1, k + 1], g)
    c10, c11 = lerp(t[i + 1, j, k], t[i + 1, j, k + 1], g), lerp(t[i + 1, j + 1, k], t[i + 1, j + 1, k + 1], g)
    return np.exp2(lerp(lerp(c00, c01, b), lerp(c10, c11, b), a)).astype(f32)


def load_header(path=None):
    """the committed table and its constants: (float32 array [NV, NY, NP], dict)"""
    import re
    path = path or os.path.join(ROOT, "trajectory_controller_amd", "csrc", "mpc_queue_key_table.h")
    text = open(path).read()
    dims = {k: int(re.search(r"kQueueKey%s = (\d+);" % k, text).group(1)) for k in ("NV", "NY", "NP", "Samples")}
    body = text[text.index("kQueueKeyTable["):]
    body = body[body.index("{") + 1:body.index("};")]
    vals = np.array([float(t) for t in re.findall(r"(-?\d+\.\d+)f", body)], dtype=np.float32)
    return vals.reshape(dims["NV"], dims["NY"], dims["NP"]), dims


def emit(table, samples, out=sys.stdout):
    nv, ny, np_ = table.shape
    w = out.write
    w("// GENERATED by scripts/gen_queue_key_table.py %d %d %d %d (`make regen`) -- do not edit.\n" % (nv, ny, np_, samples))
    w("// log2 of dlib's iteration count at N = %d over (log v, dy, dphi): the queue key of the fp64 N = %d coordinate-descent\n" % (H, H))
    w("// kernel (mpc_queue_key.h, mpc_ub.h).  Node [i][j][k] is the mean over %d seeded instances of its cell, counts from\n" % samples)
    w("// oracle/mpc_oracle.c.  Valid for EXACTLY the parameters below (the reference controller's); the host compares.\n")
    w("#pragma once\n\nnamespace tpc {\n\n")
    w("constexpr int kQueueKeyH = %d;\n" % H)
    w("constexpr int kQueueKeyNV = %d;\nconstexpr int kQueueKeyNY = %d;\nconstexpr int kQueueKeyNP = %d;\n" % (nv, ny, np_))
    w("constexpr int kQueueKeySamples = %d;\n" % samples)
    w("constexpr unsigned long long kQueueKeySeed = 0x%xull;\n" % SEED)
    w("// the box: v [m/s], dy [m], dphi [rad]\n")
    w("constexpr double kQueueKeyVLo = %r, kQueueKeyVHi = %r, kQueueKeyDyMax = %r, kQueueKeyDphiMax = %r;\n" % (V_LO, V_HI, DY_MAX, DPHI_MAX))
    w("// above the box the lookup continues the speed axis with its last cell's slope: up to this speed, that many nodes\n")
    w("constexpr double kQueueKeyVCap = %r;\nconstexpr int kQueueKeyVBeyond = %d;\n" % (V_CAP, v_beyond(table.shape)))
    lo32, scale32 = axis_consts(table.shape)
    w("// the lookup's axes (log v, dy, dphi) in float: lower face, nodes per unit\n")
    lit = lambda x: ("%.9g" % x) + ("" if any(ch in "%.9g" % x for ch in ".e") else ".0") + "f"   # noqa: E731
    w("constexpr float kQueueKeyAxisLo[3] = {%s, %s, %s};\n" % tuple(lit(x) for x in lo32))
    w("constexpr float kQueueKeyAxisScale[3] = {%s, %s, %s};\n" % tuple(lit(x) for x in scale32))
    w("// the parameters the counts were made with: weights (y, phi, front, rear), T, l, bounds, eps, max_iter, smo_iters\n")
    w("constexpr double kQueueKeyWeights[4] = {%r, %r, %r, %r};\n" % WEIGHTS)
    w("constexpr double kQueueKeyStep = %r, kQueueKeyWheelbase = %r;\n" % (STEP, WHEELBASE))
    w("constexpr double kQueueKeyLower = %s, kQueueKeyUpper = %s;   // -+22 degrees\n" % ((-ALPHA_MAX).hex(), ALPHA_MAX.hex()))
    w("constexpr double kQueueKeyEps = %r;\n" % EPS)
    w("constexpr unsigned long long kQueueKeyMaxIter = %d, kQueueKeySmoIters = %d;\n\n" % (MAX_ITER, SMO_ITERS))
    w("// (static: every translation unit that looks a key up has its own copy; under hipcc the copy is the device's)\n")
    w("#if defined(__HIPCC__)\n__device__\n#endif\n")
    w("static const float kQueueKeyTable[%d][%d][%d] = {\n" % (nv, ny, np_))
    for i in range(nv):
        w("  {   // v = %.4f\n" % math.exp(math.log(V_LO) + i * (math.log(V_HI) - math.log(V_LO)) / (nv - 1)))
        for j in range(ny):
            w("    {" + ", ".join("%.7ff" % x for x in table[i, j]) + "},\n")
        w("  },\n")
    w("};\n\n}  // namespace tpc\n")


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    shape = tuple(a[:3]) if len(a) >= 3 else SHAPE
    samples = a[3] if len(a) >= 4 else SAMPLES
    emit(make_table(shape, samples), samples)
