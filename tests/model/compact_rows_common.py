"""tests/model/compact_rows_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the CPU and GPU tests of the exact compact solve with per-instance parameters
(tpc_mpc_solve_batch_compact_exact_rows and its backward pass) share: the two recipes of per-instance parameters, the
general form of the instances built in numpy exactly as compact_exact_common.expand builds it with T, l and the rest as
rows, the chain rule of compact_grad_common with T and l as rows, and columns that make an instance invalid.
"""
import numpy as np

from tests.model.compact_exact_common import AMAX, NAMES, bits  # noqa: F401  (re-exported to the tests)
from tests.model.compact_grad_common import expanded_gradient
from trajectory_controller_amd import capi

RECIPES = ("weights", "all")
W, T, L, LO, HI = slice(0, 4), 4, 5, slice(6, 8), slice(8, 10)      # the rows of params_rows


def shared_rows(p, n):
    """p's ten model values (capi.Params) as constant rows [10, n], in the order of COMPACT_PARAM_NAMES"""
    col = [p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear, p.step_size, p.wheelbase,
           p.lower[0], p.lower[1], p.upper[0], p.upper[1]]
    return np.ascontiguousarray(np.tile(np.array(col, dtype=np.float64)[:, None], (1, n)))


def recipe_rows(recipe, H, n):
    """params_rows [10, n] of a recipe: "all" draws weights, T, l and the bounds per instance, "weights" the weights
    alone (the rest keeps default_params' values); the draws come in this order from default_rng(1000 + H)"""
    rng = np.random.default_rng(1000 + H)
    rows = shared_rows(capi.default_params(H), n)
    w = np.array([20, 7, 0.0005, 10])[:, None] * np.exp(0.5 * rng.standard_normal((4, n)))
    T_ = rng.uniform(0.05, 0.15, n)
    l_ = rng.uniform(0.15, 0.35, n)
    lo = -AMAX * rng.uniform(0.5, 1, (2, n))
    hi = AMAX * rng.uniform(0.5, 1, (2, n))
    rows[W] = w
    if recipe == "all":
        rows[T], rows[L], rows[LO], rows[HI] = T_, l_, lo, hi
    else:
        assert recipe == "weights"
    return rows


def expand(rows, H, v, dy, dphi):
    """the general form of the instances, SoA: compact_exact_common.expand with every parameter a row"""
    n = v.shape[0]
    Tv = rows[T] * v
    one, zero = np.ones(n), np.zeros(n)
    return dict(A=np.stack([one, Tv, zero, one]), B=np.stack([zero, Tv, Tv / rows[L], -(Tv / rows[L])]),
                C=np.zeros((2, n)), Q=np.ascontiguousarray(rows[0:2]), R=np.ascontiguousarray(rows[2:4]),
                lo=np.ascontiguousarray(rows[LO]), hi=np.ascontiguousarray(rows[HI]), x0=np.zeros((2, n)),
                targets=np.tile(np.stack([dy, dphi]), (H, 1)))


def chain_rule(rows, H, v, d):
    """compact_grad_common.chain_rule with T and l as rows: the outputs of the rows backward from the general
    backward's dict d, operation for operation"""
    T_, l_ = rows[T], rows[L]
    S = d["A"][1] + d["B"][1]
    D = d["B"][2] - d["B"][3]
    Tv = T_ * v
    n = v.shape[0]
    sa, sb = np.zeros(n), np.zeros(n)
    for t in range(H - 1, -1, -1):
        sa = sa + d["targets"][2 * t]
        sb = sb + d["targets"][2 * t + 1]
    out = np.stack([d["Q"][0], d["Q"][1], d["R"][0], d["R"][1],
                    v * S + (v / l_) * D,
                    -((Tv / l_) / l_) * D,
                    d["lower"][0], d["lower"][1], d["upper"][0], d["upper"][1]])
    return {"v": T_ * S + (T_ / l_) * D, "delta_y": sa, "delta_phi": sb, "params_rows": out,
            "kkt_residual": d["kkt_residual"]}


def reference(solver, rows, H, v, dy, dphi, seq, gf=None, gr=None, gs=None):
    """solve_batch_general_backward on the per-instance expanded arrays with the same sequence and g, pushed through
    chain_rule; returns (dict, flags)"""
    th = expand(rows, H, v, dy, dphi)
    d = solver.solve_batch_general_backward(*[th[k] for k in NAMES], seq, expanded_gradient(H, v.shape[0], gf, gr, gs),
                                            inputs=2)
    return chain_rule(rows, H, v, d), solver.last_flags


# what makes instance k invalid (or not): name -> (row, value or None for v, the flag it must raise, 0: legal)
INVALID = {
    # a NaN also fails the comparisons of dlib's requires clause, as it does in the general form: both flags
    "nan_weight": (1, np.nan, capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL),
    "negative_q": (0, -1.0, capi.FLAG_BAD_MODEL),
    "zero_r": (3, 0.0, capi.FLAG_BAD_MODEL),
    "upper_below_lower": (8, -1.0, capi.FLAG_BAD_MODEL),        # upper[0] = -1 < lower[0]
    "zero_wheelbase": (5, 0.0, capi.FLAG_NONFINITE),
    "infinite_v": (None, np.inf, capi.FLAG_NONFINITE),
    "infinite_bound": (9, np.inf, 0),                           # legal, and must be solved
}


def spoil(rows, v, at):
    """copies of (rows, v) with the seven cases of INVALID at the instances at[0..6], in INVALID's order"""
    rows, v = rows.copy(), v.copy()
    for (row, value, _), k in zip(INVALID.values(), at):
        if row is None:
            v[k] = value
        else:
            rows[row, k] = value
    return rows, v
