"""CPU tests of the table-predicted queue key (csrc/mpc_queue_key.h, csrc/mpc_queue_key_table.h,
scripts/gen_queue_key_table.py): the lookup the fp64 N = 20 coordinate-descent kernel calls, compiled for the host and
exported as tpc_mpc_x_queue_key_predict, against a numpy trilinear interpolation of the committed table; the committed
table against its generator; and the point of it all -- the key orders instances by iteration count better than
float(lambda) does.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_queue_key_table as qk   # noqa: E402

H = 20

# Lookup against numpy.  Both run the same float32 operations in the same order on the same constants; what may differ is
# logf and exp2f (two libraries, each within an ulp or so).  An ulp of log v (|log v| <= 2.3: 2.4e-7) moves the position on
# the speed axis by 8.4 times that, 2e-6 of a node spacing; neighbouring nodes differ by less than one unit of log2(count),
# so log2(count) moves by < 2e-6, the count by a relative 1.4e-6; an ulp of exp2f adds 1.2e-7.  A position that lands on the
# other side of a node changes nothing: the interpolant is continuous.  Held to 1e-5.
LOOKUP_RTOL = 1e-5


@pytest.fixture(scope="module")
def table():
    return qk.load_header()[0]


def _lookup(v, dy, dphi):
    from trajectory_controller_amd import capi
    lib = capi.load_library()
    v, dy, dphi = (np.ascontiguousarray(a, dtype=np.float64) for a in (v, dy, dphi))
    out = np.empty(v.shape[0], dtype=np.float32)
    rc = lib.tpc_mpc_x_queue_key_predict(v.ctypes.data, dy.ctypes.data, dphi.ctypes.data, v.shape[0], out.ctypes.data)
    assert rc == capi.OK
    return out


def _points():
    rng = np.random.default_rng(20)
    inside = np.stack([np.exp(rng.uniform(np.log(qk.V_LO), np.log(qk.V_HI), 400)), rng.uniform(-qk.DY_MAX, qk.DY_MAX, 400),
                       rng.uniform(-qk.DPHI_MAX, qk.DPHI_MAX, 400)], axis=1)
    corners = np.array([[a, b, c] for a in (qk.V_LO, qk.V_HI) for b in (-qk.DY_MAX, qk.DY_MAX) for c in (-qk.DPHI_MAX, qk.DPHI_MAX)])
    outside = np.array([[0.05, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 0.1, 0.1], [-1.0, 0.1, 0.1], [1.0, 0.7, 0.0], [1.0, -3.0, 0.0],
                        [1.0, 0.0, 0.9], [1.0, 0.0, -2.0], [9.0, 9.0, 9.0], [1e-300, -1e300, 1e300], [1e300, 1e300, -1e300]])
    bad = []
    for col in range(3):
        for val in (np.inf, -np.inf, np.nan):
            p = [1.3, 0.2, -0.3]
            p[col] = val
            bad.append(p)
    bad.append([np.nan, np.nan, np.nan])
    return inside, corners, outside, np.array(bad)


def test_lookup_matches_numpy_trilinear(table):
    for pts in _points():
        got = _lookup(pts[:, 0], pts[:, 1], pts[:, 2])
        want = qk.predict(table, pts[:, 0], pts[:, 1], pts[:, 2])
        assert np.all(np.isfinite(got)) and np.all(got >= 1.0)
        np.testing.assert_allclose(got, want, rtol=LOOKUP_RTOL, atol=0)


def test_lookup_corners_and_clamps(table):
    """a corner of the box is a node; a target outside, or a speed below, reads what its clamped image reads; a speed above
    reads what kQueueKeyVCap's does at the latest; a NaN reads the lower face"""
    _, corners, _, _ = _points()
    node = np.exp2(np.array([table[i, j, k] for i in (0, -1) for j in (0, -1) for k in (0, -1)], dtype=np.float64))
    np.testing.assert_allclose(_lookup(corners[:, 0], corners[:, 1], corners[:, 2]), node, rtol=LOOKUP_RTOL)
    raw = np.array([[0.05, 2.0, -1.5], [3.0, -0.9, 0.61], [np.inf, np.inf, -np.inf], [1e300, 0.1, 0.1], [np.nan, np.nan, np.nan]])
    img = np.array([[0.1, 0.5, -0.6], [3.0, -0.5, 0.6], [qk.V_CAP, 0.5, -0.6], [qk.V_CAP, 0.1, 0.1], [0.1, -0.5, -0.6]])
    assert np.array_equal(_lookup(raw[:, 0], raw[:, 1], raw[:, 2]), _lookup(img[:, 0], img[:, 1], img[:, 2]))


def test_speed_above_the_box_is_continued(table):
    """above kQueueKeyVHi log2(count) goes on along log v with the last cell's slope: at every target the key at 4.5, 6, 10
    and 16 m/s is the straight line through the last two nodes of the speed axis (the same float32 interpolation, its
    weight above 1: held like the lookup, plus the line's own rounding at up to 13 spacings -- 1e-4) and grows with the
    speed, as the count does -- the faster such an instance, the further ahead of the box's own it goes"""
    rng = np.random.default_rng(21)
    dy, dphi = rng.uniform(-0.7, 0.7, 200), rng.uniform(-0.8, 0.8, 200)
    _, _, d = qk.axes(table.shape)
    face = np.log2(_lookup(np.full(200, qk.V_HI), dy, dphi).astype(np.float64))
    prev = np.log2(_lookup(np.full(200, np.exp(np.log(qk.V_HI) - d[0])), dy, dphi).astype(np.float64))
    assert qk.v_beyond(table.shape) >= np.log(qk.V_CAP / qk.V_HI) / d[0]
    last = face
    for v in (4.5, 6.0, 10.0, qk.V_CAP):
        got = np.log2(_lookup(np.full(200, v), dy, dphi).astype(np.float64))
        np.testing.assert_allclose(got, face + np.log(v / qk.V_HI) / d[0] * (face - prev), rtol=1e-4)
        assert np.all(got > last)
        last = got


def test_committed_table_matches_generator(table):
    """a handful of cells recomputed from the seeded samples with the checker.  The committed entry is a float32 printed
    with seven decimals (values 7 .. 11.6: half a unit in the last printed place is 5e-8, an ulp 9.5e-7), the mean
    of log2 is taken in fp64 (differences between libraries' log2: ~1e-15): two float32 ulps."""
    _, dims = qk.load_header()
    assert table.shape == (dims["NV"], dims["NY"], dims["NP"]) and dims["Samples"] == qk.SAMPLES and table.shape == qk.SHAPE
    cells = [(0, 0, 0), (31, 11, 11), (5, 3, 8), (17, 6, 5), (24, 0, 11), (30, 9, 2)]
    flat = np.ravel_multi_index(np.array(cells).T, table.shape)
    want = qk.cell_values(flat, table.shape, dims["Samples"], nthreads=4)
    got = np.array([table[c] for c in cells], dtype=np.float64)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)


def _lambda(v, weights=qk.WEIGHTS, T=qk.STEP, l=qk.WHEELBASE):
    """dlib's trace bound for the compact model (mpc.h:116-123; csrc/mpc_ub_model.h, ctor_lambda_qdiag), vectorised"""
    q0, q1, r0, r1 = weights
    a, c = T * v, T * v / l
    lam = np.full_like(v, (r0 + r1) * H)
    z = np.zeros_like(v)
    t00, t01, t10, t11 = z + q0, z, z, z + q1
    for _ in range(H):
        p0 = c * t11 * c                                               # B = [0 a; c -c], columns (0, c) and (a, -c)
        p1 = (a * t00 - c * t10) * a + (a * t01 - c * t11) * (-c)
        lam = lam + (p0 + p1)
        u00, u01, u10, u11 = t00, t01, a * t00 + t10, a * t01 + t11   # trans(A) * t, A = [1 a; 0 1]
        t00, t01, t10, t11 = u00 + q0, u00 * a + u01, u10, u10 * a + u11 + q1
    return lam


def _midranks(x):
    order = np.argsort(x, kind="stable")
    xs = np.asarray(x)[order]
    first = np.r_[True, xs[1:] != xs[:-1]]
    start = np.flatnonzero(first)
    end = np.r_[start[1:], len(xs)]
    mid = (start + end - 1) / 2.0
    r = np.empty(len(xs))
    r[order] = np.repeat(mid, end - start)
    return r


def _spearman(a, b):
    return float(np.corrcoef(_midranks(a), _midranks(b))[0, 1])


def test_key_orders_better_than_lambda(table):
    """the first 4 096 instances of the synthetic N = 20 stream, counts from the checker: Spearman correlation of either
    key with the count, the two compared with one another (no fixed threshold)"""
    from oracle.bindings import Oracle
    from trajectory_controller_amd.synth import compact_inputs
    v, dy, dphi = compact_inputs(H, 4096)
    _, _, it = Oracle().solve_compact(H, v, dy, dphi, nthreads=4)
    lam = _lambda(v).astype(np.float32)
    assert np.all(np.diff(lam[np.argsort(v)]) >= 0)   # (lambda is a function of the speed, and a monotone one)
    key = _lookup(v, dy, dphi)
    s_lambda, s_table = _spearman(lam, it), _spearman(key, it)
    print(f"Spearman with the iteration count: float(lambda) {s_lambda:.4f}, table key {s_table:.4f}")
    assert s_table > s_lambda


def test_header_records_the_reference_parameters():
    """the constants the host compares a handle's parameters against are the library's own defaults"""
    from trajectory_controller_amd import capi
    p = capi.default_params(H, capi.F64, capi.ALGO_AUTO)
    assert (p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear) == qk.WEIGHTS
    assert (p.step_size, p.wheelbase, p.eps, p.max_iter, p.smo_iters) == (qk.STEP, qk.WHEELBASE, qk.EPS, qk.MAX_ITER, qk.SMO_ITERS)
    assert tuple(p.lower) == (-qk.ALPHA_MAX, -qk.ALPHA_MAX) and tuple(p.upper) == (qk.ALPHA_MAX, qk.ALPHA_MAX)
    text = open(os.path.join(ROOT, "trajectory_controller_amd", "csrc", "mpc_queue_key_table.h")).read()
    assert f"kQueueKeyUpper = {qk.ALPHA_MAX.hex()}" in text and f"kQueueKeyLower = {(-qk.ALPHA_MAX).hex()}" in text
