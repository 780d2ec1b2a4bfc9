"""tests/model/full_models.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

General-form instances whose 2x2 model is FULL: every entry of A and of B is live.  synth.general_inputs gives
A = [1, Tv; 0, 1] (a10 == 0, a00 == a11 == 1) and, with two inputs, b00 == 0; a kernel that drops or mis-signs an a10
term, exchanges a00 and a11 or forgets b00 is invisible on it.  Here Q, R, the bounds, x0, C and the targets stay those
of general_inputs and A is replaced per instance by class k % 6:

  0  rho * rotation(theta), rho in [0.85, 1.04], theta in [0.05, 0.6]                (complex pair)
  1  V diag(l1, l2) V^-1, l in [0.3, 0.95]^2                                         (stable, real)
  2  the same with l1 in [1.0, 1.05], l2 in [0.5, 1.0]                               (mildly unstable)
  3  the same with l1 in [0.6, 1.0], l2 in [-0.9, -0.3]                              (negative determinant)
  4  [1, a; e, 1], a in [0.05, 0.4], e in [-0.02, 0.02]                              (the shipped model, just off it)
  5  outer(a, b) scaled to a spectral radius in [0.3, 0.9]                           (rank one: singular)

V is standard normal, redrawn until cond(V) < 4 and every |a_ij| >= 0.01 (nearly equal eigenvalues would give
A ~ l I, a dead a10 again).  In class 4 the pair (a, e) is redrawn while 1 + sqrt(a e) > 1.05: the
ranges alone would allow a spectral radius of 1.089, and the family promises <= 1.05.  B is the synthetic B plus, on
every entry, a value of magnitude in [0.02, 0.2] and random sign.  tests/test_full_models_host.py asserts what the
family promises, so that no test on it passes vacuously.
"""
from __future__ import annotations

import numpy as np

from trajectory_controller_amd.synth import general_inputs

NAMES = ("A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets")
CLASSES = 6
RADIUS_CAP = 1.05
LIVE = 0.01            # smallest |a_ij| of classes 0 to 3 (class 4's e and class 5 go below)


def _eig_form(rng, r1, r2):
    """V diag(l1, l2) V^-1 with l1, l2 uniform in the ranges r1, r2; V and the eigenvalues are redrawn together"""
    while True:
        V = rng.standard_normal((2, 2))
        if np.linalg.cond(V) >= 4.0:
            continue
        A = V @ np.diag([rng.uniform(*r1), rng.uniform(*r2)]) @ np.linalg.inv(V)
        if np.abs(A).min() >= LIVE:          # nearly equal eigenvalues give A ~ l I: a10 would be dead again
            return A


def model_of_class(c, rng):
    """One 2x2 A of class c (row-major [a00, a01, a10, a11])."""
    if c == 0:
        rho, th = rng.uniform(0.85, 1.04), rng.uniform(0.05, 0.6)
        A = rho * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    elif c == 1:
        A = _eig_form(rng, (0.3, 0.95), (0.3, 0.95))
    elif c == 2:
        A = _eig_form(rng, (1.0, 1.0499), (0.5, 1.0))
    elif c == 3:
        A = _eig_form(rng, (0.6, 1.0), (-0.9, -0.3))
    elif c == 4:
        while True:
            a, e = rng.uniform(0.05, 0.4), rng.uniform(-0.02, 0.02)
            if 1.0 + np.sqrt(max(a * e, 0.0)) <= 1.049:
                break
        A = np.array([[1.0, a], [e, 1.0]])
    else:
        while True:
            a, b = rng.standard_normal(2), rng.standard_normal(2)
            if abs(a @ b) > 0.3 and min(np.abs(a).min(), np.abs(b).min()) > 0.1:
                break
        A = np.outer(a, b) * (rng.uniform(0.3, 0.9) / abs(a @ b))   # the one non-zero eigenvalue is b . a
    return A.reshape(4)


def full_models(I, H, n, seed=0):
    """The nine AoS arrays of general_inputs (same names, same shapes) with full per-instance A and B."""
    g = general_inputs(H, n, I=I, first=610000 + 4096 * seed)
    rng = np.random.default_rng([0xF011, I, H, seed])
    g["A"] = np.stack([model_of_class(k % CLASSES, rng) for k in range(n)])
    g["B"] = g["B"] + rng.uniform(0.02, 0.2, g["B"].shape) * rng.choice([-1.0, 1.0], g["B"].shape)
    return {k: np.ascontiguousarray(g[k]) for k in NAMES}


def model_class(n):
    return np.arange(n) % CLASSES


def spectral_radius(A):
    return np.abs(np.linalg.eigvals(np.asarray(A).reshape(-1, 2, 2))).max(axis=1)


def full_plant(g, s, seed=3, steps=0):
    """An ADDITIVE mismatch around the controller's model: Ap = A + s N, Bp = B + s N, Cp = C + s N with standard
    normal N (AoS, shaped like A, B, C), so the plant's a10 and b00 are live whatever the model's are.  With steps > 0
    a disturbance [n, steps, 2] = 0.1 s N comes fourth."""
    rng = np.random.default_rng([0xF012, seed])
    plant = tuple(g[k] + s * rng.standard_normal(g[k].shape) for k in ("A", "B", "C"))
    if steps:
        return plant + (0.1 * s * rng.standard_normal((g["A"].shape[0], steps, 2)),)
    return plant


def hostile(g, I):
    """The off-the-common-path instances of tests/test_ub_model.py::hostile_general on a full-model batch (in place):
    pinned and one-sided boxes, a dead input column, Q = 0, large targets."""
    from tests.test_ub_model import hostile_general
    return hostile_general(g, I)


def warm_start(I, H, n, seed=0):
    """(controls_in, v_in) [n, H, I]: controls partly outside the synthetic box of +-0.384, and a random v."""
    rng = np.random.default_rng([0xF013, I, H, seed])
    return rng.uniform(-0.45, 0.45, size=(n, H, I)), rng.uniform(-0.3, 0.3, size=(n, H, I))


def new_last_targets(g, steps, seed=0):
    """[n, steps, 2]: the last target of each instance plus a small step-wise move (what make_golden_r02.py does)."""
    rng = np.random.default_rng([0xF014, seed])
    n = g["A"].shape[0]
    return g["targets"][:, -1:, :] + (rng.uniform(size=(n, steps, 2)) - 0.5) * 0.1


def soa(a):
    """AoS [n, ...] -> the library's component-major [components, n]"""
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(a.shape[0], -1).T)
