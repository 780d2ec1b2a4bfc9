"""tests/model/compact_loop_grad_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the CPU and GPU tests of the compact closed loop's backward pass (tpc_mpc_rollout_compact_exact_backward) share:
the recorded forward (tpc_mpc_rollout_compact_exact on a host-only handle, fallback "none", computed once per case and
never modified), a random incoming gradient, the reference -- tpc_mpc_rollout_backward on the expanded arrays
(compact_loop_common.expanded, new_last_targets = None) at those records, pushed through compact_grad_common.chain_rule's
lines with dx0 taken from its "x0" -- and the per-step terms of the two target sums, obtained without the entry under
test.
"""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

from tests.model import compact_grad_common as cg
from tests.model import compact_loop_common as cl
from tests.model.compact_exact_common import NAMES, VARIANTS, bits  # noqa: F401  (re-exported to the tests)
from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import compact_inputs

ALL = ("v", "delta_y", "delta_phi", "x0", "params", "params_rows", "kkt_residual")
PER_INSTANCE = ("v", "delta_y", "delta_phi", "x0", "params_rows", "kkt_residual")
EXACT = ("v", "x0", "params_rows", "kkt_residual")      # equal to the reference as numbers; the target sums are sums


@functools.lru_cache(maxsize=None)
def records(H, S, variant="default", n=512, with_x0=False, tol=cl.TOL, rounds=cl.ROUNDS):
    """(v, dy, dphi, x0 | None, sequences, states, status) of the forward on a host-only handle; shared, read-only"""
    v, dy, dphi = compact_inputs(H, n)
    x0 = cl.start_states(H, n) if with_x0 else None
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        r = cl.loop(s, S, v, dy, dphi, x0, tol=tol, rounds=rounds)
    out = (v, dy, dphi, x0, r["sequences"], r["states"], r["status"])
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
fma = np.frompyfunc(lambda a, b, c: _libm.fma(a, b, c), 3, 1)      # C's fma(), element by element


def grads_in(S, n, seed, controls=True, states=True):
    """a random incoming gradient: (grad_controls [2S, n] | None, grad_states [2S, n] | None)"""
    rng = np.random.default_rng(seed)
    gc, gs = rng.standard_normal((2 * S, n)), rng.standard_normal((2 * S, n))
    return (gc if controls else None), (gs if states else None)


def general_backward(s, S, H, v, dy, dphi, x0, seq, states, gc, gs, **kw):
    """(the expanded arrays, rollout_backward's dict on them at the records)"""
    th = cl.expanded(s._params(), H, v, dy, dphi, x0)
    d = s.rollout_backward(S, *[th[k] for k in NAMES], None, sequences=seq, states=states, grad_controls=gc,
                           grad_states=gs, inputs=2, **kw)
    return th, d


def reference(s, S, H, v, dy, dphi, x0, seq, states, gc, gs):
    """the compact backward's per-instance outputs from the general backward, operation for operation; returns
    (dict, the general dict, flags).  "delta_y" / "delta_phi" are chain_rule's own order over the 2H dtargets rows."""
    th, d = general_backward(s, S, H, v, dy, dphi, x0, seq, states, gc, gs)
    flags = s.last_flags
    out = cg.chain_rule(s._params(), H, v, d)
    out["x0"] = d["x0"]
    return out, d, flags


def target_terms(s, S, H, v, dy, dphi, x0, seq, states, gc, gs):
    """The S*H terms of each target sum, [S*H, n] for delta_y and for delta_phi, without the entry under test: mu_kk is
    the disturbance gradient of rollout_backward with the controller's own arrays as the plant, g0 = B' mu + G_u[kk]
    is formed here with C's fma() as the sweep's line has it (an unfused g0 is one ulp off, which at S * H = 3 terms
    is as large as the bound), and each step's own dtargets comes from solve_batch_general_backward at (x_kk, U_kk,
    g0 on row 0)."""
    n = v.shape[0]
    th = cl.expanded(s._params(), H, v, dy, dphi, x0)
    model = [th[k] for k in NAMES]
    mu = s.rollout_backward(S, *model, None, sequences=seq, states=states, grad_controls=gc, grad_states=gs, inputs=2,
                            plant=(th["A"], th["B"], th["C"]), disturbance=np.zeros((2 * S, n)),
                            want=("disturbance",))["disturbance"]
    B = th["B"]
    ty, tp = [], []
    for kk in range(S):
        g = np.zeros((2 * H, n))
        for j in range(2):
            gu = np.zeros(n) if gc is None else gc[2 * kk + j]
            g[j] = fma(B[j], mu[2 * kk], fma(B[2 + j], mu[2 * kk + 1], gu)).astype(np.float64)
        step = dict(th)
        step["x0"] = th["x0"] if kk == 0 else np.ascontiguousarray(states[2 * kk - 2:2 * kk])
        dt = s.solve_batch_general_backward(*[step[k] for k in NAMES], np.ascontiguousarray(seq[2 * H * kk:2 * H * (kk + 1)]),
                                            g, inputs=2, want=("targets",))["targets"]
        ty.append(dt[0::2])
        tp.append(dt[1::2])
    return np.concatenate(ty), np.concatenate(tp)


def fsum_cols(rows):
    """math.fsum down every column of rows [r, n]"""
    rows = np.asarray(rows, dtype=np.float64)
    return np.array([math.fsum(rows[:, k]) for k in range(rows.shape[1])])


def target_bound(terms):
    """two summation orders of the same S*H terms differ by at most 2 (S*H - 1) 2^-53 sum|terms| to first order; 1 %
    on top"""
    terms = np.asarray(terms, dtype=np.float64)
    return 2.0 * (terms.shape[0] - 1) * 2.0 ** -53 * np.abs(terms).sum(axis=0) * 1.01


def ascending(rows):
    acc = np.zeros(rows.shape[0])
    for k in range(rows.shape[1]):
        acc = acc + rows[:, k]
    return acc
