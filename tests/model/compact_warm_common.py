"""tests/model/compact_warm_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the CPU and GPU tests of the warm-started exact compact solve (tpc_mpc_solve_batch_compact_exact_from) share: the
models a case runs (a shared variant of compact_exact_common.VARIANTS or a rows recipe of compact_rows_common), the same
model with its four weights moved by a step of an optimiser (+, -, +, - by `rel`), the starts, and the raw ctypes call
(the only way to pass sequence_out == start).
"""
import ctypes as C

import numpy as np

from tests.model import compact_rows_common as cr
from tests.model.compact_exact_common import NAMES, ROUNDS, TOL, VARIANTS, expand
from trajectory_controller_amd import capi

SIGNS = np.array([1.0, -1.0, 1.0, -1.0])
WEIGHTS = ("weight_y", "weight_phi", "weight_steering_front", "weight_steering_rear")
STARTS = ("moved", "random", "zeros")


def model(kind, name, H, n, rel=0.0, steps=1):
    """{"over": keyword overrides of the solver's parameters, "rows": params_rows or None} of a case: kind "shared" with
    a name of VARIANTS, or kind "rows" with a recipe; the four weights multiplied `steps` times by 1 + rel * SIGNS"""
    scale = (1.0 + rel * SIGNS) ** steps
    if kind == "rows":
        rows = cr.recipe_rows(name, H, n)
        rows[cr.W] = rows[cr.W] * scale[:, None]
        return dict(over={}, rows=rows)
    assert kind == "shared"
    over = dict(VARIANTS[name])
    p = capi.default_params(H, **over)
    for w, f in zip(WEIGHTS, scale):
        over[w] = getattr(p, w) * f
    return dict(over=over, rows=None)


def solve(s, m, v, dy, dphi, start=None, rounds=ROUNDS, fallback="none", **kw):
    """(front, rear, sequence, status, fell_back, residual_in, residual_out) of model m, cold or from `start`"""
    return s.solve_batch_compact_exact(v, dy, dphi, tol=TOL, max_rounds=rounds, fallback=fallback, want_sequence=True,
                                       want_residuals=True, params_rows=m["rows"], start=start, **m["over"], **kw)


def expanded(s, m, H, v, dy, dphi):
    """the general form of the instances of model m, as the parents' tests build it"""
    if m["rows"] is not None:
        return cr.expand(m["rows"], H, v, dy, dphi)
    return expand(s._params(**m["over"]), H, v, dy, dphi)


def polish(s, m, H, v, dy, dphi, start):
    """tpc_mpc_polish_batch_general(controls = start) on the expanded arrays: (controls, status, res_in, res_out)"""
    th = expanded(s, m, H, v, dy, dphi)
    u = np.array(start, dtype=np.float64, order="C", copy=True)
    _, st, rin, rout = s.polish_batch_general(*[th[k] for k in NAMES], u, tol=TOL, max_rounds=ROUNDS, inputs=2)
    return u, st, rin, rout


def random_start(H, n, seed):
    """finite sequences that reach outside every box the tests use (|bound| <= 0.384): the clamp is exercised"""
    return np.random.default_rng(seed).uniform(-0.6, 0.6, (2 * H, n))


def mixed_start(previous, H, seed):
    """a batch as a caller may hand it over: instance k has no start (NaN in one component, +Inf for every eighth) where
    k % 4 == 0, a random start where k % 4 == 1, and its column of `previous` otherwise"""
    n = previous.shape[1]
    start = np.array(previous, dtype=np.float64, order="C", copy=True)
    k = np.arange(n)
    rnd = k % 4 == 1
    start[:, rnd] = random_start(H, n, seed)[:, rnd]
    none = np.flatnonzero(k % 4 == 0)
    start[(none // 4) % (2 * H), none] = np.where(none % 8 == 0, np.inf, np.nan)
    return start


def raw_from(lib, h, p, v, dy, dphi, start, rows=None, rounds=ROUNDS, tol=TOL, fallback=capi.NEWTON_FALLBACK_NONE,
             in_place=False, mem=capi.HOST, stream=None, ptr=lambda a: a.ctypes.data, new=None):
    """tpc_mpc_solve_batch_compact_exact_from called directly.  in_place: sequence_out is `start` itself (which is then
    overwritten).  ptr / new adapt it to device tensors.  Returns (rc, flags, front, rear, seq, status, rin, rout)."""
    H, n = p.horizon, v.shape[0]
    new = new or (lambda dtype, rows_=None: np.empty(n if rows_ is None else (rows_, n), dtype=dtype))
    front, rear, rin, rout = (new(np.float64) for _ in range(4))
    status = new(np.int32)
    seq = start if in_place else new(np.float64, 2 * H)
    q = capi.Polish(tol=tol, max_rounds=rounds, reserved=0, status=ptr(status), residual_in=ptr(rin),
                    residual_out=ptr(rout))
    flags = C.c_uint32(99)
    rc = lib.tpc_mpc_solve_batch_compact_exact_from(
        h, C.byref(p), n, ptr(v), ptr(dy), ptr(dphi), None if rows is None else ptr(rows), ptr(start), C.byref(q),
        fallback, ptr(front), ptr(rear), ptr(seq), None, C.byref(flags), mem, stream)
    return rc, flags.value, front, rear, seq, status, rin, rout
