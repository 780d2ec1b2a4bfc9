"""CPU tests of the polish of the general form (tpc_mpc_polish_batch_general, MpcSolver.polish_batch_general) on a
host-only handle, which runs the kernel's arithmetic on the calling thread: the acceptance rule and "unchanged on
failure" against the dense checker (tests/model/mpc_polish_dense.py), the share of instances polished, optimality
against the oracle at eps 1e-10, the library against the checker over the horizons, the entry's argument and flag
behaviour, and the gradients at the polished point."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.bindings import Oracle
from tests.model import mpc_grad_dense as dense
from tests.model import mpc_polish_dense as pd
from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd.synth import general_inputs

NAMES = dense.NAMES
KEY = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets")
TOL, ROUNDS = 1e-10, 8
# (kind, I, H, n): the four inputs with a fixed share, then H = 40 and mixed_batch (no share fixed)
FIXED = [("general", 2, 4, 300), ("general", 2, 10, 300), ("general", 2, 20, 300), ("general", 1, 20, 200)]
OPEN = [("general", 2, 40, 150), ("mixed", 2, 20, 300), ("mixed", 1, 20, 300)]


@functools.lru_cache(maxsize=None)
def _inputs(kind, I, H, n):
    """(th, loose controls [n, H, I]): the model and the oracle's solution at dlib's eps 0.01"""
    if kind == "general":
        gi = general_inputs(H, n, I=I, seed=5)
        th = {k: gi[k] for k in NAMES}
    else:
        th = dense.mixed_batch(I, H, n)
    _, ctl, _ = Oracle().solve_general(I, H, *[th[k] for k in NAMES], eps=0.01)
    return th, ctl


def _polish(I, H, th, ctl, tol=TOL, rounds=ROUNDS):
    """the library on a host-only handle: (u [n, H, I], status, res_in, res_out, flags)"""
    n = ctl.shape[0]
    u = dense.soa(ctl, n).copy()
    with MpcSolver(horizon=H, device=None) as s:
        _, st, ri, ro = s.polish_batch_general(*[dense.soa(th[k], n) for k in NAMES], u, tol=tol, max_rounds=rounds,
                                               inputs=I)
        return u.T.reshape(n, H, I).copy(), st, ri, ro, s.last_flags


@pytest.mark.parametrize("kind,I,H,n", FIXED + OPEN)
def test_verified_means_verified_and_unchanged_on_failure(kind, I, H, n):
    th, ctl = _inputs(kind, I, H, n)
    u, st, ri, ro, flags = _polish(I, H, th, ctl)
    # the rounding of the two df evaluations, measured on these inputs: the dense df against dlib's recurrences at
    # the returned sequences.  Measured (max over the instances): general H=4 4.9e-14, H=10 8.9e-13, H=20 (I=2) 1.7e-11,
    # H=20 (I=1) 4.1e-12, H=40 2.6e-10; mixed H=20 I=2 2.0e-11, I=1 6.5e-12.
    slack = 0.0
    worst = 0.0
    for i in range(n):
        thi = {k: th[k][i] for k in NAMES}
        Hs, MM, lo, hi = pd.problem(I, H, thi)
        df = pd.gradient(Hs, MM, u[i].reshape(-1))
        slack = max(slack, float(np.abs(df - pd.gradient_recurrence(I, H, thi, u[i])).max()))
        if st[i] >= 0:
            worst = max(worst, pd.residual(df, pd.free_set(df, u[i].reshape(-1), lo, hi)))
    print(f"{kind} I={I} H={H}: polished {int((st >= 0).sum())}/{n}, df rounding {slack:.3e}, worst dense res {worst:.3e}")
    assert worst <= TOL + 4 * slack, (worst, slack)
    assert np.all(ro[st >= 0] <= TOL)
    assert np.all(ro <= ri)
    # unchanged on failure, bit for bit
    assert np.array_equal(u[st < 0].view(np.uint64), ctl[st < 0].view(np.uint64))
    assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((st < 0).any())
    assert flags & ~capi.FLAG_NOT_POLISHED == 0
    if (kind, I, H, n) in FIXED:
        # a condition, not a measurement: the bare Newton rule alone reaches 300, 299, 299 of 300 and 200 of 200
        assert (st >= 0).sum() >= 0.99 * n, int((st >= 0).sum())


def test_max_rounds_zero_only_verifies():
    kind, I, H, n = FIXED[1]
    th, ctl = _inputs(kind, I, H, n)
    u, st, ri, ro, flags = _polish(I, H, th, ctl, rounds=0)
    assert np.all(ri > TOL), "the eps 0.01 input is loose everywhere"
    assert np.all(st == -1) and flags == capi.FLAG_NOT_POLISHED
    assert np.array_equal(u.view(np.uint64), ctl.view(np.uint64)) and np.array_equal(ri, ro)
    # an already optimal input: status 0, the same bytes, no flag
    opt, st1, _, _, _ = _polish(I, H, th, ctl)
    ok = st1 >= 0
    sub = {k: th[k][ok] for k in NAMES}
    u2, st2, ri2, ro2, flags2 = _polish(I, H, sub, opt[ok], rounds=0)
    assert np.all(st2 == 0) and flags2 == 0
    assert np.array_equal(u2.view(np.uint64), opt[ok].view(np.uint64)) and np.array_equal(ri2, ro2)


@pytest.mark.parametrize("kind,I,H,n", FIXED)
def test_polished_point_is_the_optimum(kind, I, H, n):
    """The reference is the oracle at eps 1e-10, max_iter 2e6 -- never the library."""
    th, ctl = _inputs(kind, I, H, n)
    u, st, _, _, _ = _polish(I, H, th, ctl)
    _, ref, _ = Oracle().solve_general(I, H, *[th[k] for k in NAMES], eps=1e-10, max_iter=2000000)
    # the rounding of the evaluation: each objective in the two summation orders, 4x the largest difference seen.
    # Measured (the 4x bound): general H=4 2.1e-14, H=10 2.8e-13, H=20 (I=2) 2.3e-12, H=20 (I=1) 1.4e-12; the largest
    # f(polished) - f(oracle) seen: 4.4e-15, 7.1e-14, 1.5e-12, 1.1e-13.
    vals = []
    for i in np.flatnonzero(st >= 0):
        prob = pd.problem(I, H, {k: th[k][i] for k in NAMES})
        Hs, MM = prob[0], prob[1]
        vals.append([pd.objective(Hs, MM, u[i].reshape(-1)), pd.objective(Hs, MM, u[i].reshape(-1), reverse=True),
                     pd.objective(Hs, MM, ref[i].reshape(-1)), pd.objective(Hs, MM, ref[i].reshape(-1), reverse=True)])
    vals = np.array(vals)
    rounding = 4 * max(np.abs(vals[:, 0] - vals[:, 1]).max(), np.abs(vals[:, 2] - vals[:, 3]).max())
    excess = (vals[:, 0] - vals[:, 2]).max()
    print(f"{kind} I={I} H={H}: objective rounding bound {rounding:.3e}, max f(polished) - f(oracle) {excess:.3e}, "
          f"max |u - u*| {np.abs(u - ref)[st >= 0].max():.3e}")
    assert excess <= rounding, (excess, rounding)


# Library against checker.  The tolerance of this comparison is 1e-8: the two differ in how they evaluate df (dense
# H u + MM against the recurrences), by up to 2.6e-10 at H = 40 (see the measurement in
# test_verified_means_verified_and_unchanged_on_failure), so a tolerance at that level would compare roundings.
CMP_TOL = 1e-8


def test_library_against_checker():
    n = 40
    excused = total = 0
    worst_ratio = 0.0
    for I in (1, 2):
        for H in (1, 2, 4, 5, 10, 20, 30, 40, 64):
            th, ctl = _inputs("mixed", I, H, n)
            u, st, _, _, _ = _polish(I, H, th, ctl, tol=CMP_TOL)
            du, ds, _, _ = pd.polish_batch(I, H, th, ctl, CMP_TOL, ROUNDS)
            # the checker's own sensitivity: the same run with H_FF perturbed by a relative 1e-15 and df evaluated a
            # second way (dlib's recurrences in numpy), since the step divides the rounding of df by H_FF
            dp, dps, _, _ = pd.polish_batch(I, H, th, ctl, CMP_TOL, ROUNDS, perturb=1e-15)
            total += n
            # the comparison's tolerance: the checker's largest sensitivity over the case's instances, margin 10x.
            # Measured, the bound per case: 1.1e-15 (H = 1), 2e-14 (H = 4), 2e-12 .. 5e-12 (H = 10), 2e-11 .. 4e-11
            # (H = 20), 4e-10 .. 8e-10 (H = 40), 4e-10 .. 2.3e-9 (H = 64); library - checker reaches at most 0.12 of it.
            both = (st >= 0) & (ds >= 0) & (dps >= 0)
            # (floored at one ulp of the box's largest |u|, 0.5: a smaller sensitivity cannot be seen in a rounded u)
            sens = max(float(np.abs(dp - du)[both].max()) if both.any() else 0.0, float(np.spacing(0.5)))
            bound = 10 * sens
            for i in range(n):
                if (st[i] >= 0) != (ds[i] >= 0):
                    prob = pd.problem(I, H, {k: th[k][i] for k in NAMES})
                    last = du[i].reshape(-1) if ds[i] >= 0 else u[i].reshape(-1)
                    df = pd.gradient(prob[0], prob[1], last)
                    res = pd.residual(df, pd.free_set(df, last, prob[2], prob[3]))
                    assert abs(res - CMP_TOL) <= 0.1 * CMP_TOL, (I, H, i, st[i], ds[i], res)
                    excused += 1
                elif both[i]:
                    err = float(np.abs(u[i] - du[i]).max())
                    worst_ratio = max(worst_ratio, err / bound)
                    assert err <= bound, (I, H, i, err, bound)
            print(f"I={I} H={H}: sensitivity bound {bound:.3e}")
    print(f"library against checker: {excused} of {total} excused, worst error / bound {worst_ratio:.3f}")
    assert excused <= 0.02 * total, (excused, total)


def _raw(h, H, I, n, ld, ins, u, tol=1e-9, rounds=8, status=None, rin=None, rout=None, u0=None, dtype=capi.F64,
         mem=capi.HOST, controls=True, q=True):
    p = capi.default_params(H if 1 <= H <= 64 else 20, dtype=dtype)
    p.horizon = H
    ptr = lambda a: None if a is None else a.ctypes.data
    io = capi.GeneralIO(inputs=I, n=n, ld=ld, A=ptr(ins["A"]), B=ptr(ins["B"]), C=ptr(ins["C"]), Q=ptr(ins["Q"]),
                        R=ptr(ins["R"]), lower=ptr(ins["lo"]), upper=ptr(ins["hi"]), x0=ptr(ins["x0"]),
                        targets=ptr(ins["targets"]), controls_inout=ptr(u) if controls else None, u0=ptr(u0))
    qq = capi.Polish(tol=tol, max_rounds=rounds, status=ptr(status), residual_in=ptr(rin), residual_out=ptr(rout))
    flags = C.c_uint32(0)
    rc = capi.load_library().tpc_mpc_polish_batch_general(h, C.byref(p), C.byref(io), C.byref(qq) if q else None,
                                                          C.byref(flags), mem, None)
    return rc, flags.value


def _wide(I, H, n, ld, pad=np.nan):
    th, ctl = _inputs("mixed", I, H, n)

    def wide(a):
        a = dense.soa(a, n)
        w = np.full((a.shape[0], ld), pad)
        w[:, :n] = a
        return w
    return {k: wide(th[k]) for k in NAMES}, wide(ctl)


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


@pytest.mark.parametrize("I", [1, 2])
def test_padding_null_status_and_u0(host_handle, I):
    H, n, ld, sentinel = 7, 9, 13, 12345.0
    ins, u = _wide(I, H, n, ld)                      # the padding of the inputs (NaN) is never read
    u[:, n:] = sentinel
    st = np.full(ld, -7, dtype=np.int32)
    rin, rout, u0 = np.full(ld, sentinel), np.full(ld, sentinel), np.full((I, ld), sentinel)
    full = u.copy()
    assert _raw(host_handle, H, I, n, ld, ins, full, status=st, rin=rin, rout=rout, u0=u0) == (0, 0)
    assert np.all(st[:n] >= 0) and np.all(st[n:] == -7)
    assert np.all(full[:, n:] == sentinel) and np.all(rin[n:] == sentinel) and np.all(rout[n:] == sentinel)
    assert np.all(u0[:, n:] == sentinel) and np.array_equal(u0[:, :n], full[:I, :n])
    assert np.all(rout[:n] <= 1e-9) and np.all(rout[:n] <= rin[:n])
    bare = u.copy()                                  # every optional output NULL: the same sequence
    assert _raw(host_handle, H, I, n, ld, ins, bare) == (0, 0)
    assert np.array_equal(bare[:, :n], full[:, :n])


@pytest.mark.parametrize("what,flag", [("targets", capi.FLAG_NONFINITE), ("controls", capi.FLAG_NONFINITE),
                                       ("x0", capi.FLAG_NONFINITE), ("R", capi.FLAG_BAD_MODEL),
                                       ("bounds", capi.FLAG_BAD_MODEL)])
def test_flagged_instances_are_left_alone(host_handle, what, flag):
    I, H, n, bad = 2, 6, 5, 2
    ins, u = _wide(I, H, n, n)
    clean, st0 = u.copy(), np.zeros(n, dtype=np.int32)
    assert _raw(host_handle, H, I, n, n, ins, clean, status=st0) == (0, 0)
    if what == "targets":
        ins["targets"][3, bad] = np.nan
    elif what == "controls":
        u[H * I - 1, bad] = np.inf
    elif what == "x0":
        ins["x0"][1, bad] = -np.inf
    elif what == "R":
        ins["R"][1, bad] = 0.0
    else:
        ins["hi"][0, bad] = ins["lo"][0, bad] - 0.1
    got, st, u0 = u.copy(), np.zeros(n, dtype=np.int32), np.zeros((I, n))
    rc, flags = _raw(host_handle, H, I, n, n, ins, got, status=st, u0=u0)
    assert rc == 0 and flags == flag      # NOT_POLISHED is for the instances that were run
    assert st[bad] == -1 and np.array_equal(got[:, bad].view(np.uint64), u[:, bad].view(np.uint64))
    assert np.array_equal(u0[:, bad].view(np.uint64), u[:I, bad].view(np.uint64))
    others = [k for k in range(n) if k != bad]
    assert np.array_equal(got[:, others], clean[:, others]) and np.array_equal(st[others], st0[others])


def test_argument_errors(host_handle):
    I, H, n = 2, 4, 3
    ins, u = _wide(I, H, n, n)
    lib = capi.load_library()
    before = u.copy()
    rc, _ = _raw(host_handle, H, I, n, n, ins, u, dtype=capi.F32)
    assert rc == 1 and b"fp64" in lib.tpc_mpc_last_error(host_handle)
    for kw in (dict(tol=0.0), dict(tol=-1e-9), dict(tol=np.nan), dict(rounds=-1), dict(controls=False), dict(q=False)):
        assert _raw(host_handle, H, I, n, n, ins, u, **kw)[0] == 1, kw
    assert _raw(host_handle, 65, I, n, n, ins, u)[0] == 4
    assert _raw(host_handle, H, I, n, n - 1, ins, u)[0] == 1
    assert _raw(host_handle, H, I, n, n, ins, u, mem=capi.DEVICE)[0] == 6
    assert np.array_equal(u, before)


@pytest.mark.parametrize("I,H", [(1, 4), (2, 10), (2, 20)])
def test_gradients_at_the_polished_point(I, H):
    """solve at eps 0.01, polish, differentiate: the gradients of the optimum (the dense reference at the oracle's
    eps-1e-12 solution moved onto its stationary point), for the instances where both have the same active set, at
    the tolerance tests/test_grad_host.py holds the host path to (1e-8, normwise)."""
    n = 12
    th, ctl = _inputs("mixed", I, H, n)
    u, st, _, _, _ = _polish(I, H, th, ctl, tol=1e-9)
    _, ustar, keep = dense.solved(I, H, th)
    g = np.random.default_rng(3).standard_normal((n, H, I))
    with MpcSolver(horizon=H, device=None) as s:
        out = s.solve_batch_general_backward(*[dense.soa(th[k], n) for k in NAMES], dense.soa(u, n), dense.soa(g, n),
                                             inputs=I)
    checked = 0
    for i in np.flatnonzero(keep & (st >= 0)):
        if not np.array_equal(dense.active(u[i], th["lo"][i], th["hi"][i]),
                              dense.active(ustar[i], th["lo"][i], th["hi"][i])):
            continue
        ref, _, cond, _ = dense.instance(I, H, {k: th[k][i] for k in NAMES}, ustar[i], g[i])
        for k in NAMES:
            err = np.linalg.norm(out[KEY[k]][:, i] - ref[k].ravel())
            assert err <= 1e-8 * np.linalg.norm(ref[k]) + 1e-300, (i, k, err, cond)
        checked += 1
    assert checked >= n // 2, checked
