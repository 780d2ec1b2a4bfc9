"""tests/model/mpc_polish_dense.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Dense CPU restatement of tpc_mpc_polish_batch_general (include/tpc_mpc.h), one instance at a
time in numpy fp64: dlib's df = H u + MM from the dense hessian() of mpc_grad_dense.py, dlib's mask (mpc.h:298-299),
and the Newton step on the free set by numpy.linalg.solve -- the same step rule, safeguard included, as
csrc/mpc_polish_model.h, which gets the same step from a masked Riccati sweep.
Arrays are AoS per instance as in mpc_grad_dense.py; a sequence is [H, I].
"""
from __future__ import annotations

import numpy as np
import torch

from tests.model import mpc_grad_dense as dense

NAMES = dense.NAMES


def problem(I, H, th):
    """(Hs [HI, HI], MM [HI], lo [HI], hi [HI]) of one instance (th: dict of AoS numpy inputs)."""
    T = {k: torch.tensor(np.asarray(th[k], dtype=np.float64)) for k in NAMES}
    Hs, MM = dense.hessian(T["A"].reshape(2, 2), T["B"].reshape(2, I), T["C"], T["Q"], T["R"], T["x0"],
                           T["targets"].reshape(H, 2))
    lo = np.tile(np.asarray(th["lo"], dtype=np.float64), H)
    hi = np.tile(np.asarray(th["hi"], dtype=np.float64), H)
    return Hs.numpy(), MM.numpy(), lo, hi


def gradient(Hs, MM, u):
    return Hs @ u + MM


def gradient_recurrence(I, H, th, u):
    """df [H*I] by dlib's two recurrences (mpc.h:255-283) in plain numpy: x_{t+1} = A x_t + B u_t + C forward, then
    p_t = A' p_{t+1} + Q (x_{t+1} - target_t), df_t = B' p_t + R u_t backward.  A second evaluation of the quantity
    gradient() computes, in the order of operations the library uses: the distance between the two is the rounding of
    a df evaluation on the given inputs."""
    A = np.asarray(th["A"], dtype=np.float64).reshape(2, 2)
    B = np.asarray(th["B"], dtype=np.float64).reshape(2, I)
    u = np.asarray(u, dtype=np.float64).reshape(H, I)
    tg = np.asarray(th["targets"], dtype=np.float64).reshape(H, 2)
    x = np.asarray(th["x0"], dtype=np.float64)
    xs = []
    for t in range(H):
        x = A @ x + B @ u[t] + th["C"]
        xs.append(x)
    p = np.zeros(2)
    df = np.empty((H, I))
    for t in range(H - 1, -1, -1):
        p = A.T @ p + th["Q"] * (xs[t] - tg[t])
        df[t] = B.T @ p + th["R"] * u[t]
    return df.reshape(H * I)


def free_set(df, u, lo, hi):
    """dlib's mask: blocked iff on a bound with the gradient pushing outward, or pinned (lower == upper)."""
    blocked = ((u <= lo) & (df > 0)) | ((u >= hi) & (df < 0)) | (lo == hi)
    return ~blocked


def residual(df, F):
    return float(np.abs(df[F]).max()) if F.any() else 0.0


def objective(Hs, MM, u, reverse=False):
    """1/2 u'Hu + MM'u with every sum -- the rows of H u and the final one -- accumulated in index order, or all of them
    in the reverse order (the two orders bound the rounding of the evaluation)."""
    idx = np.arange(u.size)[::-1] if reverse else np.arange(u.size)
    acc = 0.0
    for i in idx:
        row = 0.0
        for j in idx:
            row += float(Hs[i, j]) * float(u[j])
        acc += float(u[i]) * (0.5 * row + float(MM[i]))
    return acc


def polish(prob, u_in, tol, max_rounds, perturb=0.0, df_of=None):
    """The shipped rule on one instance.  Returns (u [H*I], status, res_in, res_out): status = rounds used, or -1 with u
    = u_in.  The checker's own sensitivity probe: `perturb` scales H_FF by (1 + perturb) entrywise-random, and `df_of`
    (u -> df) replaces the dense df by a second evaluation of it (gradient_recurrence)."""
    Hs, MM, lo, hi = prob
    u0 = np.asarray(u_in, dtype=np.float64).reshape(-1)
    u = np.minimum(np.maximum(u0, lo), hi)
    rng = np.random.default_rng(12345)
    res_in = prev = None
    inner = False
    for rnd in range(max_rounds + 1):
        df = gradient(Hs, MM, u) if df_of is None else df_of(u)
        F = free_set(df, u, lo, hi)
        res = residual(df, F)
        if rnd == 0:
            res_in = res
        if not np.isfinite(df).all():
            break
        if res <= tol:
            return u, rnd, res_in, res
        if rnd == max_rounds:
            break
        # safeguard: after a round that did not lower the residual, one round steps only the components strictly
        # inside the box (those on a bound stay), then dlib's mask is used again
        inner = (not inner) and prev is not None and not (res < prev)
        if inner:
            F = F & (u > lo) & (u < hi)
        prev = res
        if F.any():
            HFF = Hs[np.ix_(F, F)]
            if perturb:
                HFF = HFF * (1.0 + perturb * rng.uniform(-1.0, 1.0, HFF.shape))
            w = np.linalg.solve(HFF, df[F])
            u = u.copy()
            u[F] = np.minimum(np.maximum(u[F] - w, lo[F]), hi[F])
    return u0.copy(), -1, res_in, res_in


def polish_batch(I, H, th, controls, tol, max_rounds, perturb=0.0):
    """controls [n, H, I] -> (u [n, H, I], status [n], res_in [n], res_out [n])"""
    n = controls.shape[0]
    out = np.empty((n, H * I))
    st = np.empty(n, dtype=np.int32)
    ri = np.empty(n)
    ro = np.empty(n)
    for i in range(n):
        thi = {k: th[k][i] for k in NAMES}
        df_of = (lambda u: gradient_recurrence(I, H, thi, u)) if perturb else None
        out[i], st[i], ri[i], ro[i] = polish(problem(I, H, thi), controls[i], tol, max_rounds, perturb, df_of)
    return out.reshape(n, H, I), st, ri, ro
