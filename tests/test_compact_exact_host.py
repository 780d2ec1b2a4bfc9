"""CPU tests of the exact compact solve (tpc_mpc_solve_batch_compact_exact, MpcSolver.solve_batch_compact_exact) on a
host-only handle, which runs the kernel's arithmetic on the calling thread with TPC_MPC_NEWTON_FALLBACK_NONE: the bits
against tpc_mpc_polish_batch_general on the expanded arrays with zero controls, the share the Newton rounds verify from
a cold start, optimality of what they verify, the rows of what they do not, non-finite inputs and the argument checks.

n = 4096 instances of compact_inputs(H, 4096), tol 1e-9, max_rounds 16.  The expanded arrays are built in numpy exactly
as mpc_compact (autograd.py) builds them in torch: Tv = T * v, B = [0, Tv, Tv / l, -Tv / l].

The objective comparison against the oracle at eps 1e-10 takes every verified instance at every horizon but H = 64,
where it takes a fixed sample, every 128th instance (32 of 4096): the oracle is a first-order method, needs about 1e5
iterations per instance at H = 40 and at H = 64 stops on its cap of 2e6 iterations on part of the batch, which costs
the most and still gives a valid one-sided reference (f(exact) <= f(oracle) must hold all the more).  The dense
residual -- the proof of optimality -- is checked on every verified instance at every horizon."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle.bindings import Oracle
from tests.model import mpc_grad_dense as dense
from tests.model import mpc_polish_dense as pd
from tests.model.compact_exact_common import N, NAMES, ROUNDS, TOL, VARIANTS, bits, expand
from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd.synth import compact_inputs

assert NAMES == dense.NAMES
HS = (1, 4, 5, 7, 10, 20, 40, 64)
# unverified of 4096 after 16 rounds by tpc_mpc_polish_batch_general(controls = 0) before this entry existed
PARENT_UNVERIFIED = {4: 0, 5: 0, 10: 38, 20: 125, 40: 189}
ORACLE_STRIDE = {64: 128}      # H -> every how-manyth instance meets the oracle (default: every one)


@functools.lru_cache(maxsize=None)
def _case(H, variant="default", rounds=ROUNDS):
    """the entry and the polish on the expanded arrays, one run each, shared by the tests (never modified)"""
    v, dy, dphi = compact_inputs(H, N)
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        front, rear, seq, st, fb, rin, rout = s.solve_batch_compact_exact(
            v, dy, dphi, tol=TOL, max_rounds=rounds, fallback="none", want_sequence=True, want_residuals=True)
        flags = s.last_flags
        th = expand(s.params, H, v, dy, dphi)
        u = np.zeros((2 * H, N))
        _, pst, prin, prout = s.polish_batch_general(*[th[k] for k in NAMES], u, tol=TOL, max_rounds=rounds, inputs=2)
        pflags = s.last_flags
    assert fb is None
    return dict(front=front, rear=rear, seq=seq, st=st, rin=rin, rout=rout, flags=flags, th=th,
                pu=u, pst=pst, prin=prin, prout=prout, pflags=pflags)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("H", HS)
def test_bits_equal_the_polish_on_the_expanded_arrays(H, variant):
    c = _case(H, variant)
    ok = c["st"] >= 0
    print(f"H={H} {variant}: verified {int(ok.sum())}/{N}, mean rounds {c['st'][ok].mean() if ok.any() else 0:.3f}")
    assert np.array_equal(c["st"], c["pst"])
    assert np.array_equal(bits(c["seq"]), bits(c["pu"]))          # signed zeros included
    assert np.array_equal(bits(c["front"]), bits(c["pu"][0])) and np.array_equal(bits(c["rear"]), bits(c["pu"][1]))
    assert np.array_equal(bits(c["rin"]), bits(c["prin"]))
    assert np.array_equal(bits(c["rout"][ok]), bits(c["prout"][ok]))
    assert c["flags"] == c["pflags"]


@pytest.mark.parametrize("H", sorted(PARENT_UNVERIFIED))
def test_coverage_from_a_cold_start(H):
    c = _case(H)
    unverified = int((c["st"] < 0).sum())
    ok = c["st"] >= 0
    print(f"H={H}: unverified {unverified}/{N} ({100.0 * unverified / N:.2f} %), mean rounds of the verified "
          f"{c['st'][ok].mean():.2f}, histogram {np.bincount(c['st'][ok], minlength=ROUNDS + 1).tolist()}")
    if H in (4, 5):
        assert unverified == 0
    else:
        assert unverified <= 0.10 * N
    assert unverified == PARENT_UNVERIFIED[H]


def _df_recurrence(th, u, H):
    """pd.gradient_recurrence for the whole batch: dlib's two recurrences, SoA [component, n] -> df [2H, n]"""
    a, b, c, q, r, tg = th["A"], th["B"], th["C"], th["Q"], th["R"], th["targets"]
    x0, x1 = th["x0"]
    xs = []
    for t in range(H):
        x0, x1 = (a[0] * x0 + a[1] * x1 + b[0] * u[2 * t] + b[1] * u[2 * t + 1] + c[0],
                  a[2] * x0 + a[3] * x1 + b[2] * u[2 * t] + b[3] * u[2 * t + 1] + c[1])
        xs.append((x0, x1))
    p0 = p1 = np.zeros_like(x0)
    df = np.empty_like(u)
    for t in range(H - 1, -1, -1):
        p0, p1 = (a[0] * p0 + a[2] * p1 + q[0] * (xs[t][0] - tg[2 * t]),
                  a[1] * p0 + a[3] * p1 + q[1] * (xs[t][1] - tg[2 * t + 1]))
        df[2 * t] = b[0] * p0 + b[2] * p1 + r[0] * u[2 * t]
        df[2 * t + 1] = b[1] * p0 + b[3] * p1 + r[1] * u[2 * t + 1]
    return df


def _dense_problem(th, H, sel):
    """dense.hessian (what pd.problem calls) for the instances sel at once: Hs [m, 2H, 2H], MM [m, 2H]"""
    t = lambda k, *shape: torch.tensor(np.ascontiguousarray(th[k][:, sel].T)).reshape(-1, *shape)
    Hs, MM = torch.func.vmap(dense.hessian)(t("A", 2, 2), t("B", 2, 2), t("C", 2), t("Q", 2), t("R", 2), t("x0", 2),
                                            t("targets", H, 2))
    return Hs.numpy(), MM.numpy()


def _objective(Hs, MM, u, reverse=False):
    """pd.objective for a batch: the same sums in the same order, every instance at once (u [m, 2H])"""
    idx = np.arange(u.shape[1])[::-1] if reverse else np.arange(u.shape[1])
    acc = np.zeros(u.shape[0])
    for i in idx:
        row = np.zeros(u.shape[0])
        for j in idx:
            row += Hs[:, i, j] * u[:, j]
        acc += u[:, i] * (0.5 * row + MM[:, i])
    return acc


def _objective_rounding(Hs, MM, u):
    """A priori bound of one evaluation's rounding, per instance: every term passes through at most 2 * 2H + 3 rounded
    operations (a row sum of 2H products, the halving, + MM, the product with u_i, the outer sum of 2H terms), so the
    error is at most (4H + 3) * 2^-53 of the sum of the terms' magnitudes (recursive summation, first order).  Used
    at H = 1 only, where the two-orders measure reads 0: a sum of two terms has no second order."""
    terms = np.abs(u) * (0.5 * np.einsum("mij,mj->mi", np.abs(Hs), np.abs(u)) + np.abs(MM))
    return (2 * u.shape[1] + 3) * 2.0 ** -53 * terms.sum(axis=1)


@pytest.mark.parametrize("H", HS)
def test_verified_instances_are_the_optimum(H):
    c = _case(H)
    th, st, u = c["th"], c["st"], c["seq"]
    lo, hi = np.tile(th["lo"], (H, 1)), np.tile(th["hi"], (H, 1))
    # ---- dense residual of every verified instance, with the allowance of tests/test_polish_host.py: the rounding of
    # the two df evaluations (dense H u + MM against dlib's recurrences) at the returned sequences, 4x
    rec = _df_recurrence(th, u, H)
    worst = slack = 0.0
    for first in range(0, N, 512):
        sel = np.arange(first, min(first + 512, N))
        Hs, MM = _dense_problem(th, H, sel)
        df = np.einsum("mij,mj->mi", Hs, u[:, sel].T) + MM
        if first == 0:    # the batched evaluation is the checker's own, instance by instance
            prob = pd.problem(2, H, {k: th[k][:, 0] for k in NAMES})
            assert np.allclose(prob[0], Hs[0], rtol=1e-12, atol=0) and np.allclose(prob[1], MM[0], rtol=1e-12, atol=0)
            assert _objective(prob[0][None], prob[1][None], u[:, :1].T)[0] == pd.objective(prob[0], prob[1], u[:, 0])
        slack = max(slack, float(np.abs(df.T - rec[:, sel]).max()))
        F = pd.free_set(df.T, u[:, sel], lo[:, sel], hi[:, sel])
        res = np.where(F, np.abs(df.T), 0.0).max(axis=0)
        v = st[sel] >= 0
        worst = max(worst, float(res[v].max()) if v.any() else 0.0)
    print(f"H={H}: verified {int((st >= 0).sum())}/{N}, df rounding {slack:.3e}, worst dense residual {worst:.3e}")
    assert worst <= TOL + 4 * slack, (worst, slack)
    assert np.all(c["rout"][st >= 0] <= TOL)

    # ---- objective against the oracle at eps 1e-10, max_iter 2e6 (never the library), up to the rounding of the
    # evaluation: each objective in the two summation orders, 4x the largest difference seen (test_polish_host.py),
    # at H = 1, where that measure is 0, the a priori bound of the two evaluations (_objective_rounding)
    take = np.arange(0, N, ORACLE_STRIDE.get(H, 1))
    m = take.size
    aos = {k: np.ascontiguousarray(th[k][:, take].T) for k in NAMES}
    _, ref, _ = Oracle().solve_general(2, H, *[aos[k] for k in NAMES], eps=1e-10, max_iter=2000000,
                                       nthreads=min(8, os.cpu_count() or 1))
    ref = ref.reshape(m, 2 * H)
    excess, rounding = -np.inf, 0.0
    for first in range(0, m, 512):
        at = np.arange(first, min(first + 512, m))
        sel = take[at]
        v = st[sel] >= 0
        Hs, MM = _dense_problem(th, H, sel)
        Hs, MM, mine, theirs = Hs[v], MM[v], u[:, sel].T[v], ref[at][v]
        f = [_objective(Hs, MM, mine), _objective(Hs, MM, mine, reverse=True),
             _objective(Hs, MM, theirs), _objective(Hs, MM, theirs, reverse=True)]
        rounding = max(rounding, 4 * float(np.abs(f[0] - f[1]).max()), 4 * float(np.abs(f[2] - f[3]).max()))
        if H == 1:
            rounding = max(rounding, float((_objective_rounding(Hs, MM, mine) + _objective_rounding(Hs, MM, theirs)).max()))
        excess = max(excess, float((f[0] - f[2]).max()))
    print(f"H={H}: {m} instances against the oracle, objective rounding bound {rounding:.3e}, "
          f"max f(exact) - f(oracle) {excess:.3e}")
    assert excess <= rounding, (excess, rounding)


@pytest.mark.parametrize("H", [10, 20, 64])
def test_unverified_rows_are_zeros(H):
    c = _case(H)
    bad = c["st"] < 0
    assert bad.any() and np.all(c["st"][bad] == -1)
    zero = np.zeros(int(bad.sum()), dtype=np.uint64)                 # +0.0, bit for bit
    assert np.array_equal(bits(c["front"][bad]), zero) and np.array_equal(bits(c["rear"][bad]), zero)
    assert not bits(c["seq"][:, bad]).any() and np.array_equal(bits(c["rout"][bad]), zero)
    assert np.all(c["rin"][bad] > TOL)
    assert c["flags"] == capi.FLAG_NOT_POLISHED
    assert _case(4)["flags"] == 0


@pytest.mark.parametrize("H", [4, 20])
def test_nonfinite_inputs_are_flagged_and_not_counted_as_unverified(H):
    clean = _case(H)
    v, dy, dphi = (a.copy() for a in compact_inputs(H, N))
    ok = np.flatnonzero(clean["st"] >= 0)
    k = ok[[3, 700, 2500]]                  # three verified instances: NaN speed, +inf and -inf targets
    v[k[0]], dy[k[1]], dphi[k[2]] = np.nan, np.inf, -np.inf
    with MpcSolver(horizon=H, device=None) as s:
        front, rear, seq, st, _, rin, rout = s.solve_batch_compact_exact(
            v, dy, dphi, tol=TOL, max_rounds=ROUNDS, fallback="none", want_sequence=True, want_residuals=True)
        flags = s.last_flags
    assert flags == capi.FLAG_NONFINITE | clean["flags"]     # H = 4: NONFINITE alone, no NOT_POLISHED of their own
    assert np.all(st[k] == -1) and not bits(front[k]).any() and not bits(rear[k]).any()
    assert not bits(seq[:, k]).any() and not bits(rin[k]).any() and not bits(rout[k]).any()
    rest = np.setdiff1d(np.arange(N), k)
    assert np.array_equal(st[rest], clean["st"][rest]) and np.array_equal(bits(seq[:, rest]), bits(clean["seq"][:, rest]))
    assert int((st < 0).sum()) == int((clean["st"] < 0).sum()) + 3


def test_max_rounds_zero_only_verifies():
    c = _case(10, rounds=0)
    assert np.array_equal(c["st"], c["pst"]) and np.array_equal(bits(c["rin"]), bits(c["prin"]))
    assert np.all(c["st"] == -1) and c["flags"] == capi.FLAG_NOT_POLISHED and not bits(c["seq"]).any()
    # a zero target is optimal at U = 0: verified in round 0, nothing else run
    z = np.zeros(5)
    with MpcSolver(horizon=10, device=None) as s:
        front, rear, st, fb = s.solve_batch_compact_exact(np.linspace(0.5, 3.0, 5), z, z, max_rounds=0, fallback="none")
        assert np.all(st == 0) and s.last_flags == 0 and not bits(front).any() and not bits(rear).any()


def _raw(h, n=3, H=4, q=True, tol=TOL, rounds=ROUNDS, fallback=capi.NEWTON_FALLBACK_NONE, mem=capi.HOST,
         dtype=capi.F64, null=None, **over):
    p = capi.default_params(H if 1 <= H <= 64 else 20, dtype=dtype, **over)
    p.horizon = H
    v, dy, dphi = compact_inputs(4, max(n, 1))
    front, rear = np.full(max(n, 1), 7.0), np.full(max(n, 1), 7.0)
    ptr = lambda a, name: None if null == name else a.ctypes.data
    qq = capi.Polish(tol=tol, max_rounds=rounds)
    flags = C.c_uint32(99)
    rc = capi.load_library().tpc_mpc_solve_batch_compact_exact(
        h, C.byref(p), n, ptr(v, "v"), ptr(dy, "dy"), ptr(dphi, "dphi"), C.byref(qq) if q else None, fallback,
        ptr(front, "front"), ptr(rear, "rear"), None, None, C.byref(flags), mem, None)
    return rc, flags.value, front


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


def test_degenerate_calls_and_argument_errors(host_handle):
    h = host_handle
    rc, flags, front = _raw(h)                      # the plain call, every optional output NULL
    assert (rc, flags) == (0, 0) and np.all(front != 7.0)
    rc, flags, front = _raw(h, n=0)
    assert (rc, flags) == (0, 0) and np.all(front == 7.0)
    BAD_ARG, BAD_WEIGHTS, BAD_BOUNDS, BAD_HORIZON, BAD_EPS, NO_DEVICE = 1, 2, 3, 4, 5, 6
    for kw in (dict(q=False), dict(tol=0.0), dict(tol=-1e-9), dict(tol=np.nan), dict(rounds=-1), dict(fallback=2),
               dict(fallback=-1), dict(dtype=capi.F32), dict(n=-1), dict(mem=5), dict(null="v"), dict(null="dphi"),
               dict(null="front"), dict(null="rear"), dict(step_size=np.inf), dict(wheelbase=0.0)):
        assert _raw(h, **kw)[0] == BAD_ARG, kw
    assert _raw(h, dtype=capi.F32)[0] == BAD_ARG and b"fp64" in capi.load_library().tpc_mpc_last_error(h)
    # p is validated as tpc_mpc_solve_batch_compact validates it
    assert _raw(h, weight_y=-1.0)[0] == BAD_WEIGHTS and _raw(h, weight_steering_rear=0.0)[0] == BAD_WEIGHTS
    assert _raw(h, lower=(0.1, -0.1), upper=(0.0, 0.1))[0] == BAD_BOUNDS
    assert _raw(h, H=65)[0] == BAD_HORIZON and _raw(h, H=0)[0] == BAD_HORIZON
    assert _raw(h, eps=0.0)[0] == BAD_EPS
    # a host-only handle: no fallback solve and no DEVICE memory -- reported after the argument checks
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE)[0] == NO_DEVICE
    assert _raw(h, mem=capi.DEVICE)[0] == NO_DEVICE
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE, tol=0.0)[0] == BAD_ARG
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE, n=0)[0] == NO_DEVICE
    with MpcSolver(horizon=4, device=None) as s:
        with pytest.raises(capi.TpcMpcError) as e:
            s.solve_batch_compact_exact(*compact_inputs(4, 8))           # fallback="solve" is the default
        assert e.value.status == NO_DEVICE


def test_symbol_is_declared_and_documented():
    lib = capi.load_library()
    assert "tpc_mpc_solve_batch_compact_exact" in capi.EXPORTS and hasattr(lib, "tpc_mpc_solve_batch_compact_exact")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tpc_mpc.h")) as f:
        text = f.read()
    assert "int tpc_mpc_solve_batch_compact_exact(" in text and "#define TPC_MPC_ABI_VERSION 5 " in text
