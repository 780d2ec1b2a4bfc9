"""tests/model/compact_loop_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the CPU and GPU tests of the compact closed loop (tpc_mpc_rollout_compact_exact) share: the batch, the settings
(tol 1e-9, 16 rounds), the controller models (compact_exact_common.VARIANTS) and the reference -- tpc_mpc_rollout_newton
on compact_exact_common.expand(...) with x0 put in, new_last_targets = None, controls = None and the same q.
"""
import numpy as np

from tests.model.compact_exact_common import NAMES, ROUNDS, TOL, VARIANTS, bits, expand   # noqa: F401 (re-exported)
from trajectory_controller_amd.synth import compact_inputs, splitmix64_uniform

# (H, S) of the host module's cases; n = 4096, 1024 at H >= 40
CASES = ((1, 3), (4, 8), (5, 8), (7, 5), (10, 10), (20, 10), (40, 6), (64, 3))
ROWS = ("controls", "states", "sequences", "status", "rin", "rout", "first")


def batch_size(H):
    return 1024 if H >= 40 else 4096


def start_states(H, n):
    """a random x0 [2, n] in +-0.1"""
    return np.ascontiguousarray(-0.1 + 0.2 * splitmix64_uniform(0xC100 + H, 2 * n).reshape(2, n))


def loop(s, S, v, dy, dphi, x0=None, tol=TOL, rounds=ROUNDS, fallback="none", **kw):
    """the entry: {row name: array} and "flags" """
    n = v.shape[0]
    rin, rout = np.empty((S, n)), np.empty((S, n))
    c, x, q, st, first = s.rollout_compact_exact(S, v, dy, dphi, x0, tol=tol, max_rounds=rounds, fallback=fallback,
                                                 residuals=(rin, rout), **kw)
    return dict(controls=c, states=x, sequences=q, status=st, rin=rin, rout=rout, first=first, flags=s.last_flags)


def expanded(p, H, v, dy, dphi, x0=None):
    th = expand(p, H, v, dy, dphi)
    if x0 is not None:
        th["x0"] = np.ascontiguousarray(x0, dtype=np.float64)
    return th


def reference(s, S, v, dy, dphi, x0=None, tol=TOL, rounds=ROUNDS, fallback="none", polished=False, **kw):
    """tpc_mpc_rollout_newton (polished: tpc_mpc_rollout_polished, no "first") on the expanded arrays"""
    H, n = s._params(**kw).horizon, v.shape[0]
    th = expanded(s._params(**kw), H, v, dy, dphi, x0)
    rin, rout = np.empty((S, n)), np.empty((S, n))
    if polished:
        c, x, q, st, _ = s.rollout_polished(S, *[th[k] for k in NAMES], tol=tol, max_rounds=rounds, inputs=2,
                                            residuals=(rin, rout), **kw)
        first = None
    else:
        c, x, q, st, _, first = s.rollout_newton(S, *[th[k] for k in NAMES], tol=tol, max_rounds=rounds,
                                                 fallback=fallback, inputs=2, residuals=(rin, rout), **kw)
    return dict(controls=c, states=x, sequences=q, status=st, rin=rin, rout=rout, first=first, flags=s.last_flags)


def same_rows(a, b, rows=ROWS, cols=None):
    """the names of the rows whose bytes differ (signed zeros included), over the instances cols (default: all)"""
    bad = []
    for k in rows:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if cols is not None:
            x, y = x[..., cols], y[..., cols]
        same = np.array_equal(x, y) if x.dtype == np.int32 else np.array_equal(bits(x), bits(y))
        if not same:
            bad.append(k)
    return bad
