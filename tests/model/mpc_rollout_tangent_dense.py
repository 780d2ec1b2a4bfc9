"""tests/model/mpc_rollout_tangent_dense.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Dense CPU reference of the forward-mode derivatives (tpc_mpc_rollout_forward, tpc_mpc_solve_batch_general_forward,
include/tpc_mpc.h), in torch fp64, one instance and one direction at a time: the directional derivative of
mpc_rollout_dense.closed_loop's (u0, states) -- and of mpc_grad_dense.instance's u* -- along a tangent dict, by
torch.autograd.functional.jvp on the same dense pieces (dense.hessian, the active-set solve on a given sequence's
active set, the rollout's target map).  Arrays are AoS per instance as in mpc_grad_dense; a tangent dict maps NAMES
(and "nlt" [S, 2]) to arrays shaped like the inputs, a missing name is a zero tangent.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd

NAMES = dense.NAMES


def _primals_tangents(th, extra, tan):
    keys = list(NAMES) + list(extra)
    src = dict({k: th[k] for k in NAMES}, **extra)
    prim = tuple(torch.tensor(np.asarray(src[k], dtype=np.float64)) for k in keys)
    tang = tuple(torch.tensor(np.asarray(tan[k], dtype=np.float64).reshape(p.shape)) if tan.get(k) is not None
                 else torch.zeros_like(p) for k, p in zip(keys, prim))
    return keys, prim, tang


def closed_loop_jvp(I, H, S, th, nlt, act_seqs, tan):
    """Directional derivative of the closed loop of one instance on the active sets of act_seqs [S, H, I] along tan:
    (tu0 [S, I], tstates [S, 2], u0 [S, I], states [S, 2])."""
    has_nlt = nlt is not None
    keys, prim, tang = _primals_tangents(th, {"nlt": nlt} if has_nlt else {}, tan)

    def loop(*args):
        T = dict(zip(keys, args))
        A, B = T["A"].reshape(2, 2), T["B"].reshape(2, I)
        tg, lo, hi, x = T["targets"].reshape(H, 2), T["lo"].reshape(I), T["hi"].reshape(I), T["x0"].reshape(2)
        u0s, xs = [], []
        for k in range(S):
            rows = []
            for t in range(H):
                src, r = rd.target_source(H, k, t, has_nlt)
                rows.append(tg[r] if src == "targets" else T["nlt"].reshape(S, 2)[r])
            Hs, MM = dense.hessian(A, B, T["C"], T["Q"], T["R"], x, torch.stack(rows))
            u0 = rd._active_solve(Hs, MM, lo, hi, act_seqs[k], H)[:I]
            x = A @ x + B @ u0 + T["C"]
            u0s.append(u0)
            xs.append(x)
        return torch.stack(u0s), torch.stack(xs)

    (u0, xs), (tu0, txs) = torch.autograd.functional.jvp(loop, prim, tang)
    return tu0.numpy(), txs.numpy(), u0.numpy(), xs.numpy()


def instance_jvp(I, H, th, controls, tan):
    """Directional derivative of the single solve's stationary point on the active set of controls [H, I] along tan:
    (tU [H, I], u* [H, I])."""
    keys, prim, tang = _primals_tangents(th, {}, tan)

    def solve(*args):
        T = dict(zip(keys, args))
        Hs, MM = dense.hessian(T["A"].reshape(2, 2), T["B"].reshape(2, I), T["C"], T["Q"], T["R"], T["x0"].reshape(2),
                               T["targets"].reshape(H, 2))
        return rd._active_solve(Hs, MM, T["lo"].reshape(I), T["hi"].reshape(I), controls, H)

    u, tu = torch.autograd.functional.jvp(solve, prim, tang)
    return tu.numpy().reshape(H, I), u.numpy().reshape(H, I)


def random_tangents(I, H, S, n, seed, with_nlt=True, K=1):
    """K random full directions for n instances, AoS: a list of K dicts of arrays [n, ...] keyed NAMES (+ "nlt")"""
    rng = np.random.default_rng(seed)
    shapes = dict(A=(4,), B=(2 * I,), C=(2,), Q=(2,), R=(I,), lo=(I,), hi=(I,), x0=(2,), targets=(H, 2))
    if with_nlt:
        shapes["nlt"] = (S, 2)
    return [{k: rng.standard_normal((n,) + s) for k, s in shapes.items()} for _ in range(K)]


def soa_tangents(dirs, n):
    """a list of K AoS direction dicts -> the solver's `tangents` dict of [K, c, n] arrays"""
    key = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets",
               nlt="new_last_targets")
    return {key[k]: np.stack([dense.soa(d[k], n) for d in dirs]) for k in dirs[0]}
