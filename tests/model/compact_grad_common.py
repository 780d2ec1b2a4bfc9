"""tests/model/compact_grad_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the CPU and GPU tests of the exact compact solve's backward pass (tpc_mpc_solve_batch_compact_exact_backward)
share: the incoming gradient of the expanded form, the chain rule of the model building in numpy -- the lines of
include/tpc_mpc.h, one rounded operation each -- applied to solve_batch_general_backward's dict, the a-priori bound
of a sum of n doubles, and the device's own order of that sum (device_sum).
"""
import math

import numpy as np

from tests.model.compact_exact_common import NAMES, VARIANTS, bits, expand  # noqa: F401  (re-exported to the tests)

PER_INSTANCE = ("v", "delta_y", "delta_phi", "params_rows", "kkt_residual")


def grad_in(H, n, seed, sequence=False):
    """a random incoming gradient: (grad_front, grad_rear, grad_sequence or None)"""
    rng = np.random.default_rng(seed)
    gf, gr = rng.standard_normal(n), rng.standard_normal(n)
    return gf, gr, (rng.standard_normal((2 * H, n)) if sequence else None)


def expanded_gradient(H, n, gf=None, gr=None, gs=None):
    """g [2H, n] of the definition: grad_sequence, plus grad_front at row 0 and grad_rear at row 1, in the order
    grad_sequence + grad_front; an absent array counts as +0.0"""
    g = np.zeros((2 * H, n)) if gs is None else np.array(gs, dtype=np.float64)
    g[0] = g[0] + (np.zeros(n) if gf is None else gf)
    g[1] = g[1] + (np.zeros(n) if gr is None else gr)
    return g


def chain_rule(p, H, v, d):
    """the outputs of the compact backward from the general backward's dict d (p: capi.Params), operation for operation"""
    T, l = p.step_size, p.wheelbase
    S = d["A"][1] + d["B"][1]
    D = d["B"][2] - d["B"][3]
    Tv = T * v
    n = v.shape[0]
    sa, sb = np.zeros(n), np.zeros(n)
    for t in range(H - 1, -1, -1):
        sa = sa + d["targets"][2 * t]
        sb = sb + d["targets"][2 * t + 1]
    rows = np.stack([d["Q"][0], d["Q"][1], d["R"][0], d["R"][1],
                     v * S + (v / l) * D,
                     -((Tv / l) / l) * D,
                     d["lower"][0], d["lower"][1], d["upper"][0], d["upper"][1]])
    return {"v": T * S + (T / l) * D, "delta_y": sa, "delta_phi": sb, "params_rows": rows,
            "kkt_residual": d["kkt_residual"]}


def reference(solver, H, v, dy, dphi, seq, gf=None, gr=None, gs=None, **over):
    """solve_batch_general_backward on the expanded arrays with the same sequence and g, pushed through chain_rule;
    returns (dict, flags).  `solver` takes numpy arrays (a host-only handle, or a device handle staging them)."""
    p = solver._params(**over)
    th = expand(p, H, v, dy, dphi)
    d = solver.solve_batch_general_backward(*[th[k] for k in NAMES], seq, expanded_gradient(H, v.shape[0], gf, gr, gs),
                                            inputs=2, **over)
    return chain_rule(p, H, v, d), solver.last_flags


def same_numbers(a, b):
    """equal as numbers (the sign of a zero is free; no NaN is expected on either side)"""
    return np.array_equal(np.asarray(a), np.asarray(b))


def fsum_bound(rows):
    """|any summation order of n doubles - the exact sum| <= (n - 1) * 2^-53 * sum|x| to first order; 1 % on top"""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[-1]
    return (n - 1) * 2.0 ** -53 * np.abs(rows).sum(axis=-1) * 1.01


def fsum_rows(rows):
    return np.array([math.fsum(r) for r in np.asarray(rows, dtype=np.float64)])


WAVE, REDUCE_BLOCK = 64, 256


def grad_block(n):
    """rollout_grad_block's rule: the largest of 256, 128, 64 lanes that still gives 256 blocks, else 64"""
    for b in (256, 128):
        if -(-n // b) >= 256:
            return b
    return 64


def device_sum(rows):
    """The ten doubles the device must return as "params" for the per-instance rows [10, n]: the summation order of
    mpc_compact_grad.hip (block_partials, compact_grad_reduce_kernel) in numpy fp64, one rounded addition per addition
    of the kernels.  No call into the library."""
    rows = np.asarray(rows, dtype=np.float64)
    P, n = rows.shape
    block = grad_block(n)
    blocks = -(-n // block)
    lanes = np.zeros((P, blocks * block))                   # a lane past n holds +0.0
    lanes[:, :n] = rows
    a = lanes.reshape(P, blocks * block // WAVE, WAVE)
    lane = np.arange(WAVE)
    for mask in (32, 16, 8, 4, 2, 1):                       # the butterfly: every lane ends with the same value
        a = a + a[:, :, lane ^ mask]
    waves = a[:, :, 0].reshape(P, blocks, block // WAVE)
    part = waves[:, :, 0].copy()                            # the block: wavefront 0, then 1.. in ascending order
    for w in range(1, block // WAVE):
        part = part + waves[:, :, w]
    x = np.zeros((P, REDUCE_BLOCK))                         # the reduce: thread t adds partials t, t + 256, ...
    for b0 in range(0, blocks, REDUCE_BLOCK):
        m = min(REDUCE_BLOCK, blocks - b0)
        x[:, :m] = x[:, :m] + part[:, b0:b0 + m]
    half = REDUCE_BLOCK // 2
    while half > 0:                                         # the tree: lds[t] = lds[t] + lds[t + half]
        x[:, :half] = x[:, :half] + x[:, half:2 * half]
        half >>= 1
    return np.ascontiguousarray(x[:, 0])
