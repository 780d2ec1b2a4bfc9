"""tests/model/compact_exact_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the CPU and GPU tests of the exact compact solve (tpc_mpc_solve_batch_compact_exact) share: the batch, the polish
settings, the controller models (VARIANTS), and the general form of the compact instances built in numpy exactly as
mpc_compact (autograd.py) builds it in torch: Tv = T * v, B = [0, Tv, Tv / l, -Tv / l].
"""
import numpy as np

NAMES = ("A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets")      # mpc_grad_dense.NAMES
N, TOL, ROUNDS = 4096, 1e-9, 16
AMAX = 22.0 * np.pi / 180.0
# the controller models the tests run: keyword overrides of capi.default_params
VARIANTS = {
    "default": {},
    "weights": dict(weight_y=3.0, weight_phi=11.0, weight_steering_front=0.02, weight_steering_rear=0.7,
                    step_size=0.05, wheelbase=0.3),
    "asymmetric": dict(lower=(-0.05, -0.3), upper=(0.2, 0.01)),
    "offset": dict(lower=(0.01, -0.3), upper=(0.2, -0.02)),       # U = 0 lies outside the box
    "pinned": dict(lower=(-AMAX, 0.02), upper=(AMAX, 0.02)),      # the rear input pinned (lower == upper)
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def expand(p, H, v, dy, dphi):
    """the general form of the compact instances, SoA (p: capi.Params)"""
    n = v.shape[0]
    Tv = p.step_size * v
    one, zero = np.ones(n), np.zeros(n)
    rows = lambda *x: np.ascontiguousarray(np.tile(np.array(x, dtype=np.float64)[:, None], (1, n)))
    return dict(A=np.stack([one, Tv, zero, one]), B=np.stack([zero, Tv, Tv / p.wheelbase, -Tv / p.wheelbase]),
                C=np.zeros((2, n)), Q=rows(p.weight_y, p.weight_phi),
                R=rows(p.weight_steering_front, p.weight_steering_rear), lo=rows(*p.lower), hi=rows(*p.upper),
                x0=np.zeros((2, n)), targets=np.tile(np.stack([dy, dphi]), (H, 1)))
