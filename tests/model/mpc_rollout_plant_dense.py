"""tests/model/mpc_rollout_plant_dense.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Dense CPU reference of the closed loop against a separate plant (tpc_mpc_rollout_plant and its backward / forward,
include/tpc_mpc.h), in torch fp64, one instance at a time: mpc_rollout_dense.closed_loop restated with the plant line
  x_{k+1} = Ap x_k + Bp u0_k + Cp + d_k
and torch.autograd over the extra leaves Ap [4], Bp [2I], Cp [2] and d [S, 2]; every step's QP is built from the
controller's A, B, C as before (mpc_grad_dense.hessian, mpc_rollout_dense._active_solve and target_source are
imported, not copied).  closed_loop_jvp is the directional derivative of the same function.  plant = None means the
controller's model moves the state (the plant leaves then get zero gradients); dist = None is a zero disturbance.
replay() is mpc_rollout_polish_ref.replay -- the oracle's solve, the host polish -- with the plant line.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.model import mpc_rollout_polish_ref as rp

NAMES = dense.NAMES
PLANT_NAMES = ("Ap", "Bp", "Cp", "d")


def _loop(I, H, S, T, has_nlt, has_plant, act_seqs):
    """the closed loop on a dict of torch leaves: (u0 [S, I], states [S, 2], sequences [S, H*I])"""
    A, B = T["A"].reshape(2, 2), T["B"].reshape(2, I)
    tg, lo, hi, x = T["targets"].reshape(H, 2), T["lo"].reshape(I), T["hi"].reshape(I), T["x0"].reshape(2)
    Ap, Bp, Cp = (T["Ap"].reshape(2, 2), T["Bp"].reshape(2, I), T["Cp"]) if has_plant else (A, B, T["C"])
    d = T["d"].reshape(S, 2)
    u0s, xs, seqs = [], [], []
    for k in range(S):
        rows = []
        for t in range(H):
            src, r = rd.target_source(H, k, t, has_nlt)
            rows.append(tg[r] if src == "targets" else T["nlt"].reshape(S, 2)[r])
        Hs, MM = dense.hessian(A, B, T["C"], T["Q"], T["R"], x, torch.stack(rows))
        full = rd._active_solve(Hs, MM, lo, hi, act_seqs[k], H)
        u0 = full[:I]
        x = Ap @ x + Bp @ u0 + Cp + d[k]          # the plant line
        u0s.append(u0)
        xs.append(x)
        seqs.append(full)
    return torch.stack(u0s), torch.stack(xs), torch.stack(seqs)


def _leaves(I, S, th, nlt, plant, dist):
    src = {k: th[k] for k in NAMES}
    src["nlt"] = nlt if nlt is not None else np.zeros((S, 2))
    if plant is not None:
        src.update(Ap=plant[0], Bp=plant[1], Cp=plant[2])
    else:
        src.update(Ap=np.zeros(4), Bp=np.zeros(2 * I), Cp=np.zeros(2))
    src["d"] = dist if dist is not None else np.zeros((S, 2))
    return src


def closed_loop(I, H, S, th, nlt, act_seqs, G_u, G_x, plant=None, dist=None):
    """The closed loop of one instance against the plant, on the active sets of act_seqs [S, H, I], differentiated:
    (grads, u0 [S, I], states [S, 2], sequences [S, H, I]).  grads holds NAMES, "nlt" [S, 2] and PLANT_NAMES."""
    src = _leaves(I, S, th, nlt, plant, dist)
    keys = list(src)
    T = {k: torch.tensor(np.asarray(src[k], dtype=np.float64), requires_grad=True) for k in keys}
    u0, xs, seqs = _loop(I, H, S, T, nlt is not None, plant is not None, act_seqs)
    L = (u0 * torch.tensor(np.asarray(G_u, dtype=np.float64).reshape(S, I))).sum() \
        + (xs * torch.tensor(np.asarray(G_x, dtype=np.float64).reshape(S, 2))).sum()
    grads = torch.autograd.grad(L, [T[k] for k in keys], allow_unused=True)
    out = {k: (np.zeros(np.shape(src[k])) if g is None else g.detach().numpy().reshape(np.shape(src[k])))
           for k, g in zip(keys, grads)}
    return out, u0.detach().numpy(), xs.detach().numpy(), seqs.detach().numpy().reshape(S, H, I)


def closed_loop_jvp(I, H, S, th, nlt, act_seqs, tan, plant=None, dist=None):
    """Directional derivative along tan (a dict over NAMES, "nlt" and PLANT_NAMES; a missing name is zero):
    (tu0 [S, I], tstates [S, 2], u0 [S, I], states [S, 2])."""
    src = _leaves(I, S, th, nlt, plant, dist)
    keys = list(src)
    prim = tuple(torch.tensor(np.asarray(src[k], dtype=np.float64)) for k in keys)
    tang = tuple(torch.tensor(np.asarray(tan[k], dtype=np.float64).reshape(p.shape)) if tan.get(k) is not None
                 else torch.zeros_like(p) for k, p in zip(keys, prim))

    def loop(*args):
        return _loop(I, H, S, dict(zip(keys, args)), nlt is not None, plant is not None, act_seqs)[:2]

    (u0, xs), (tu0, txs) = torch.autograd.functional.jvp(loop, prim, tang)
    return tu0.numpy(), txs.numpy(), u0.numpy(), xs.numpy()


def replay(I, H, S, th, nlt, plant, dist, eps=0.01, max_iter=10000, tol=1e-9, max_rounds=8):
    """mpc_rollout_polish_ref.replay (oracle solve, host polish) of a batch with the plant line: th AoS [n, ...],
    plant (Ap [n, 4], Bp [n, 2I], Cp [n, 2]) | None, dist [n, S, 2] | None.  (u0 [n, S, I], states [n, S, 2],
    sequences [n, S, H, I], status [n, S])"""
    from oracle.bindings import Oracle
    o = Oracle()
    n = np.asarray(th["A"]).reshape(-1, 4).shape[0]
    A, B, C = plant if plant is not None else (th["A"], th["B"], th["C"])
    A, B, C = (np.asarray(a, dtype=np.float64).reshape(n, -1) for a in (A, B, C))
    T = np.array(np.asarray(th["targets"], dtype=np.float64).reshape(n, H, 2))
    x = np.array(np.asarray(th["x0"], dtype=np.float64).reshape(n, 2))
    model = [np.asarray(th[k], dtype=np.float64) for k in NAMES[:7]]
    ctl = v = None
    u0s, xs, seqs = np.empty((n, S, I)), np.empty((n, S, 2)), np.empty((n, S, H, I))
    status = np.zeros((n, S), dtype=np.int32)
    for k in range(S):
        if k > 0:
            T[:, :-1] = T[:, 1:].copy()
            if nlt is not None:
                T[:, H - 1] = nlt[:, k]
        _, cout, _, v = o.solve_general(I, H, *model, x, T, controls_in=ctl, v_in=v, eps=eps, max_iter=max_iter,
                                        want_v=True)
        cout, status[:, k], _, _ = rp._polish_host(I, H, th, x, T, cout, tol, max_rounds)
        ctl = cout
        u = cout[:, 0]
        xn = np.empty((n, 2))
        for r in range(2):
            bu = B[:, r * I] * u[:, 0]
            if I == 2:
                bu = bu + B[:, r * I + 1] * u[:, 1]
            xn[:, r] = ((A[:, 2 * r] * x[:, 0] + A[:, 2 * r + 1] * x[:, 1]) + bu) + C[:, r]
            if dist is not None:
                xn[:, r] = xn[:, r] + dist[:, k, r]
        x = xn
        u0s[:, k], xs[:, k], seqs[:, k] = u, x, cout
    return u0s, xs, seqs, status
