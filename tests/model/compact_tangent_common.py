"""tests/model/compact_tangent_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the CPU and GPU tests of the exact compact solve's forward mode (tpc_mpc_solve_batch_compact_exact_forward) share:
random directions, the chain rule of the model building in numpy -- the four lines of include/tpc_mpc.h, one rounded
operation each -- and the expansion of a compact direction to solve_batch_general_forward's tangent dict.
"""
import numpy as np

from tests.model.compact_exact_common import NAMES, VARIANTS, bits, expand  # noqa: F401  (re-exported to the tests)

NP = 10
T, L = 4, 5                                                     # the rows of step_size and wheelbase
VECTORS = ("v", "delta_y", "delta_phi")


def directions(n, K, seed, rows=False):
    """K full random directions: "v", "delta_y", "delta_phi" [K, n] and "params" [K, 10] (rows: "params_rows"
    [K, 10, n]), every component drawn"""
    rng = np.random.default_rng(seed)
    d = {k: rng.standard_normal((K, n)) for k in VECTORS}
    if rows:
        d["params_rows"] = rng.standard_normal((K, NP, n))
    else:
        d["params"] = rng.standard_normal((K, NP))
    return d


def params_tangent(d, K, n):
    """the parameters' tangent of a direction dict as [K, 10, n], whichever key carries it (none: zeros)"""
    if "params_rows" in d:
        return np.asarray(d["params_rows"], dtype=np.float64).reshape(K, NP, n)
    if "params" in d:
        return np.ascontiguousarray(np.broadcast_to(np.asarray(d["params"], dtype=np.float64).reshape(K, NP, 1),
                                                    (K, NP, n)))
    return np.zeros((K, NP, n))


def chain_rule(T_, l_, v, tv, tT, tl):
    """tTv and ttvl of the definition, operation for operation (T_, l_: scalars or rows [n]; tv, tT, tl: [K, n])"""
    Tv = T_ * v
    tvl = Tv / l_
    tTv = tT * v + T_ * tv
    ttvl = (tTv - tvl * tl) / l_
    return tTv, ttvl


def expand_tangents(T_, l_, H, v, d, K):
    """solve_batch_general_forward's tangent dict of the compact directions d (a missing key: zeros)"""
    n = v.shape[0]
    zero = np.zeros((K, n))
    vec = {k: np.asarray(d[k], dtype=np.float64).reshape(K, n) if k in d else zero for k in VECTORS}
    tp = params_tangent(d, K, n)
    tTv, ttvl = chain_rule(T_, l_, v, vec["v"], tp[:, T], tp[:, L])
    st = lambda *x: np.ascontiguousarray(np.stack(x, axis=1))
    return dict(A=st(zero, tTv, zero, zero), B=st(zero, tTv, ttvl, -ttvl), C=np.zeros((K, 2, n)),
                Q=np.ascontiguousarray(tp[:, 0:2]), R=np.ascontiguousarray(tp[:, 2:4]),
                lower=np.ascontiguousarray(tp[:, 6:8]), upper=np.ascontiguousarray(tp[:, 8:10]),
                x0=np.zeros((K, 2, n)),
                targets=np.ascontiguousarray(np.tile(st(vec["delta_y"], vec["delta_phi"]), (1, H, 1))))


def reference(solver, th, T_, l_, H, v, seq, d, K):
    """solve_batch_general_forward on the expanded arrays th and the expanded directions: (tU [K, 2H, n], flags)"""
    tu = solver.solve_batch_general_forward(*[th[k] for k in NAMES], seq, expand_tangents(T_, l_, H, v, d, K), inputs=2)
    return tu, solver.last_flags


def same_numbers(a, b):
    """equal as numbers (the sign of a zero is free; no NaN is expected on either side)"""
    return np.array_equal(np.asarray(a), np.asarray(b))
