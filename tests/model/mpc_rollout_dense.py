"""tests/model/mpc_rollout_dense.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Dense CPU reference of the derivative that tpc_mpc_rollout_backward computes (include/tpc_mpc.h), in torch fp64, one
instance at a time, built from mpc_grad_dense's pieces:
  - step k solves from x_k with the targets T_k of the rollout's shift (target_source);
  - its sequence is the active-set solve of mpc_grad_dense (the active set fixed from a given sequence, the free
    components at the stationary point u_F = -H_FF^-1 (MM_F + H_FA u_A));
  - x_{k+1} = A x_k + B u0_k + C;
  - the gradients of L = sum G_u . controls + sum G_x . states are taken by torch.autograd.grad.
replay() is the oracle's closed loop step by step (Oracle.solve_general carrying controls and v), which also returns
every step's sequence.  Arrays are AoS per instance, as in mpc_grad_dense; nlt [S, 2].
"""
from __future__ import annotations

import numpy as np
import torch

from tests.model import mpc_grad_dense as dense

NAMES = dense.NAMES


def target_source(H, k, t, has_nlt):
    """where T_k[t] comes from: ("targets", row) or ("nlt", row)"""
    r = t + k
    if r <= H - 1:
        return "targets", r
    if has_nlt:
        return "nlt", r - (H - 1)
    return "targets", H - 1


def replay(I, H, S, th, nlt=None, eps=0.01, max_iter=10000):
    """The oracle's closed loop of one instance, one operator() call at a time: (u0 [S, I], states [S, 2],
    sequences [S, H, I], iters [S])."""
    from oracle.bindings import Oracle
    o = Oracle()
    A, B, C = (np.asarray(th[k], dtype=np.float64) for k in ("A", "B", "C"))
    T = np.array(np.asarray(th["targets"], dtype=np.float64).reshape(H, 2))
    x = np.array(np.asarray(th["x0"], dtype=np.float64).reshape(2))
    ctl = v = None
    u0s, xs, seqs, its = [], [], [], []
    for k in range(S):
        if k > 0:
            T[:-1] = T[1:].copy()      # operator()'s shift (mpc.h:236-237), then set_last_target
            if nlt is not None:
                T[H - 1] = nlt[k]
        _, cout, it, vout = o.solve_general(I, H, *[np.asarray(th[kk])[None] for kk in ("A", "B", "C", "Q", "R",
                                                                                      "lo", "hi")],
                                            x[None], T[None], controls_in=ctl, v_in=v, eps=eps, max_iter=max_iter,
                                            want_v=True)
        ctl, v = cout, vout
        u = cout[0, 0]
        xn = np.empty(2)
        for r in range(2):   # the plant update of the oracle's rollout, operation for operation
            bu = B[r * I] * u[0]
            if I == 2:
                bu = bu + B[r * I + 1] * u[1]
            xn[r] = ((A[2 * r] * x[0] + A[2 * r + 1] * x[1]) + bu) + C[r]
        x = xn
        u0s.append(u.copy())
        xs.append(x.copy())
        seqs.append(cout[0].copy())
        its.append(int(it[0]))
    return np.array(u0s), np.array(xs), np.array(seqs), np.array(its)


def _active_solve(Hs, MM, lo, hi, act_from, H):
    """mpc_grad_dense's active-set solve of one step: the sequence [H*I] on the active set of act_from [H, I]"""
    u = np.asarray(act_from, dtype=np.float64).reshape(-1)
    lo_r, hi_r = lo.repeat(H), hi.repeat(H)
    at_lo = u <= lo_r.detach().numpy()
    act = at_lo | (u >= hi_r.detach().numpy())
    F = np.flatnonzero(~act)
    Aidx = np.flatnonzero(act)
    uA = torch.where(torch.tensor(at_lo[Aidx]), lo_r[Aidx], hi_r[Aidx])
    full = torch.zeros(u.size, dtype=torch.float64)
    full = full.index_put((torch.tensor(Aidx, dtype=torch.long),), uA)
    if F.size:
        Fi = torch.tensor(F, dtype=torch.long)
        Ai = torch.tensor(Aidx, dtype=torch.long)
        rhs = MM[Fi] + (Hs[Fi][:, Ai] @ uA if Aidx.size else 0.0)
        full = full.index_put((Fi,), -torch.linalg.solve(Hs[Fi][:, Fi], rhs))
    return full


def closed_loop(I, H, S, th, nlt, act_seqs, G_u, G_x):
    """The closed loop of one instance on the active sets of act_seqs [S, H, I], differentiated: (grads, u0 [S, I],
    states [S, 2], sequences [S, H, I]).  grads holds NAMES shaped like th's arrays, and "nlt" [S, 2] (zeros without
    nlt)."""
    T = {k: torch.tensor(np.asarray(th[k], dtype=np.float64), requires_grad=True) for k in NAMES}
    has_nlt = nlt is not None
    Tn = torch.tensor(np.asarray(nlt if has_nlt else np.zeros((S, 2)), dtype=np.float64), requires_grad=True)
    A = T["A"].reshape(2, 2)
    B = T["B"].reshape(2, I)
    tg = T["targets"].reshape(H, 2)
    lo = T["lo"].reshape(I)
    hi = T["hi"].reshape(I)
    x = T["x0"].reshape(2)
    L = torch.zeros((), dtype=torch.float64)
    u0s, xs, seqs = [], [], []
    for k in range(S):
        rows = []
        for t in range(H):
            src, r = target_source(H, k, t, has_nlt)
            rows.append(tg[r] if src == "targets" else Tn.reshape(S, 2)[r])
        Tk = torch.stack(rows)
        Hs, MM = dense.hessian(A, B, T["C"], T["Q"], T["R"], x, Tk)
        full = _active_solve(Hs, MM, lo, hi, act_seqs[k], H)
        u0 = full[:I]
        x = A @ x + B @ u0 + T["C"]
        L = L + (u0 * torch.tensor(np.asarray(G_u[k], dtype=np.float64))).sum() \
              + (x * torch.tensor(np.asarray(G_x[k], dtype=np.float64))).sum()
        u0s.append(u0.detach().numpy().copy())
        xs.append(x.detach().numpy().copy())
        seqs.append(full.detach().numpy().reshape(H, I).copy())
    grads = torch.autograd.grad(L, [T[k] for k in NAMES] + [Tn], allow_unused=True)
    out = {}
    for k, gr in zip(list(NAMES) + ["nlt"], grads):
        shape = np.shape(th[k]) if k != "nlt" else (S, 2)
        out[k] = np.zeros(shape) if gr is None else gr.detach().numpy().reshape(shape)
    return out, np.array(u0s), np.array(xs), np.array(seqs)


def loss(u0s, xs, G_u, G_x):
    return float(np.sum(u0s * G_u) + np.sum(xs * G_x))


def batch(I, H, S, n, seed=0, with_nlt=True):
    """AoS inputs of n instances (mpc_grad_dense.mixed_batch: mixed active sets) and new_last_targets [n, S, 2] near
    the initial targets (or None)."""
    th = dense.mixed_batch(I, H, n, seed=seed)
    if not with_nlt:
        return th, None
    rng = np.random.default_rng(4242 + 31 * H + 7 * S + I + seed)
    last = np.asarray(th["targets"]).reshape(n, H, 2)[:, -1:, :]
    return th, last + 0.05 * rng.standard_normal((n, S, 2))
