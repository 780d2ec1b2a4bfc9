"""CPU tests of the exact compact solve with per-instance parameters (tpc_mpc_solve_batch_compact_exact_rows and
tpc_mpc_solve_batch_compact_exact_rows_backward, MpcSolver.solve_batch_compact_exact[_backward](params_rows=...)) on a
host-only handle, which runs the kernels' arithmetic on the calling thread with TPC_MPC_NEWTON_FALLBACK_NONE.

Forward: the bits against tpc_mpc_polish_batch_general(controls = 0) on the per-instance expanded arrays, constant rows
against the shared entry, the share the Newton rounds verify from a cold start as a condition, optimality of what they
verify, invalid instances.  Backward: the numbers against tpc_mpc_solve_batch_general_backward on the expanded arrays
pushed through the rows chain rule (tests/model/compact_rows_common.py), constant rows against the shared backward,
central differences of the rows forward, the batch sum.  Then the argument checks.

Coverage.  n = 4096 instances of compact_inputs(H, 4096), tol 1e-9, 16 rounds.  The unverified counts were measured with
tpc_mpc_polish_batch_general(controls = 0) on the expanded arrays before the entry existed (UNVERIFIED below); the
conditions are at most 20 % of the batch for recipe "all" (17.6 % at worst, H = 64) and at most 10 % for recipe
"weights" (6.5 % at worst, H = 40).

Finite differences.  As tests/test_compact_grad_host.py: the step of an input x is 1e-6 max(1, |x|) where |x| > 0.1 and
1e-4 |x| below; one parameter row is perturbed for all instances at once (the instances are independent); an instance
is kept if it is verified with an unchanged active set at every perturbed point; the bound is 1e-5 norm-wise."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests.model import compact_grad_common as cg
from tests.model import compact_rows_common as cr
from tests.model import mpc_polish_dense as pd
from tests.model.compact_exact_common import N, NAMES, ROUNDS, TOL, VARIANTS, bits
from tests.test_compact_exact_host import _dense_problem, _df_recurrence
from trajectory_controller_amd import COMPACT_PARAM_NAMES, MpcSolver, capi
from trajectory_controller_amd.synth import compact_inputs

HS = (1, 4, 5, 7, 10, 20, 40, 64)
NB = 512                       # the backward tests' batch
ALL = ("v", "delta_y", "delta_phi", "params", "params_rows", "kkt_residual")
# unverified of 4096 after 16 rounds by tpc_mpc_polish_batch_general(controls = 0) on the per-instance expanded arrays,
# measured before the entry existed
UNVERIFIED = {("weights", 4): 0, ("weights", 5): 8, ("weights", 10): 68, ("weights", 20): 181, ("weights", 40): 265,
              ("all", 4): 2, ("all", 5): 21, ("all", 7): 81, ("all", 10): 176, ("all", 20): 478, ("all", 40): 676,
              ("all", 64): 719}
SHARE = {"all": 0.20, "weights": 0.10}


@functools.lru_cache(maxsize=None)
def _case(H, recipe):
    """the rows entry and the polish on the expanded arrays, one run each, shared by the tests (never modified)"""
    v, dy, dphi = compact_inputs(H, N)
    rows = cr.recipe_rows(recipe, H, N)
    with MpcSolver(horizon=H, device=None) as s:
        front, rear, seq, st, fb, rin, rout = s.solve_batch_compact_exact(
            v, dy, dphi, tol=TOL, max_rounds=ROUNDS, fallback="none", want_sequence=True, want_residuals=True,
            params_rows=rows)
        flags = s.last_flags
        th = cr.expand(rows, H, v, dy, dphi)
        u = np.zeros((2 * H, N))
        _, pst, prin, prout = s.polish_batch_general(*[th[k] for k in NAMES], u, tol=TOL, max_rounds=ROUNDS, inputs=2)
        pflags = s.last_flags
    assert fb is None
    return dict(front=front, rear=rear, seq=seq, st=st, rin=rin, rout=rout, flags=flags, th=th, rows=rows,
                pu=u, pst=pst, prin=prin, prout=prout, pflags=pflags)


# ---- forward

@pytest.mark.parametrize("recipe", cr.RECIPES)
@pytest.mark.parametrize("H", HS)
def test_bits_equal_the_polish_on_the_expanded_arrays(H, recipe):
    c = _case(H, recipe)
    ok = c["st"] >= 0
    print(f"H={H} {recipe}: verified {int(ok.sum())}/{N}, mean rounds {c['st'][ok].mean() if ok.any() else 0:.3f}")
    assert np.array_equal(c["st"], c["pst"])
    assert np.array_equal(bits(c["seq"]), bits(c["pu"]))          # signed zeros included
    assert np.array_equal(bits(c["front"]), bits(c["pu"][0])) and np.array_equal(bits(c["rear"]), bits(c["pu"][1]))
    assert np.array_equal(bits(c["rin"]), bits(c["prin"]))
    assert np.array_equal(bits(c["rout"][ok]), bits(c["prout"][ok]))
    assert not bits(c["rout"][~ok]).any()
    assert c["flags"] == c["pflags"]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("H", [4, 5, 7, 20])
def test_constant_rows_equal_the_shared_entry(H, variant):
    v, dy, dphi = compact_inputs(H, N)
    kw = dict(tol=TOL, max_rounds=ROUNDS, fallback="none", want_sequence=True, want_residuals=True)
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        shared = s.solve_batch_compact_exact(v, dy, dphi, **kw)
        sflags = s.last_flags
        rows = cr.shared_rows(s.params, N)
    with MpcSolver(horizon=H, device=None) as s:                  # p's own model values are not read
        got = s.solve_batch_compact_exact(v, dy, dphi, params_rows=rows, **kw)
        assert s.last_flags == sflags
    for a, b in zip(got, shared):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


@pytest.mark.parametrize("recipe", cr.RECIPES)
@pytest.mark.parametrize("H", HS)
def test_coverage_from_a_cold_start(H, recipe):
    c = _case(H, recipe)
    unverified = int((c["st"] < 0).sum())
    ok = c["st"] >= 0
    print(f"H={H} {recipe}: unverified {unverified}/{N} ({100.0 * unverified / N:.2f} %), mean rounds of the verified "
          f"{c['st'][ok].mean():.2f}")
    assert unverified == int((c["pst"] < 0).sum())
    assert unverified <= SHARE[recipe] * N
    if (recipe, H) in UNVERIFIED:
        assert unverified == UNVERIFIED[(recipe, H)]
    assert c["flags"] == (capi.FLAG_NOT_POLISHED if unverified else 0)


@pytest.mark.parametrize("recipe", cr.RECIPES)
@pytest.mark.parametrize("H", HS)
def test_verified_instances_meet_the_dense_residual(H, recipe):
    """section 19's condition, as tests/test_compact_exact_host.py states it: the dense residual of every verified
    instance is at most tol plus the rounding of the two df evaluations (dense H u + MM against dlib's recurrences), 4x"""
    c = _case(H, recipe)
    th, st, u = c["th"], c["st"], c["seq"]
    lo, hi = np.tile(th["lo"], (H, 1)), np.tile(th["hi"], (H, 1))
    rec = _df_recurrence(th, u, H)
    worst = slack = 0.0
    for first in range(0, N, 512):
        sel = np.arange(first, min(first + 512, N))
        Hs, MM = _dense_problem(th, H, sel)
        df = np.einsum("mij,mj->mi", Hs, u[:, sel].T) + MM
        slack = max(slack, float(np.abs(df.T - rec[:, sel]).max()))
        F = pd.free_set(df.T, u[:, sel], lo[:, sel], hi[:, sel])
        res = np.where(F, np.abs(df.T), 0.0).max(axis=0)
        ok = st[sel] >= 0
        worst = max(worst, float(res[ok].max()) if ok.any() else 0.0)
    print(f"H={H} {recipe}: verified {int((st >= 0).sum())}/{N}, df rounding {slack:.3e}, worst dense residual {worst:.3e}")
    assert worst <= TOL + 4 * slack, (worst, slack)
    assert np.all(c["rout"][st >= 0] <= TOL)


def _verified_seven(st):
    return np.flatnonzero(st >= 0)[[3, 40, 100, 150, 200, 300, 400]]


@pytest.mark.parametrize("H", [4, 20])
def test_invalid_instances(H):
    clean = _case(H, "all")
    v, dy, dphi = compact_inputs(H, N)
    at = _verified_seven(clean["st"])
    rows, vv = cr.spoil(clean["rows"], v, at)
    bad, legal = at[:6], at[6]
    kw = dict(tol=TOL, max_rounds=ROUNDS, fallback="none", want_sequence=True, want_residuals=True)
    with MpcSolver(horizon=H, device=None) as s:
        front, rear, seq, st, _, rin, rout = s.solve_batch_compact_exact(vv, dy, dphi, params_rows=rows, **kw)
        # no NOT_POLISHED of their own: only what the clean batch raises
        assert s.last_flags == capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL | clean["flags"]
        # each case on its own, among verified neighbours: its flag alone
        near = np.flatnonzero(clean["st"] >= 0)[450:457]
        for (name, (_, _, flag)), k in zip(cr.INVALID.items(), at):
            sel = np.concatenate([near[:3], [k], near[3:]])
            one = s.solve_batch_compact_exact(vv[sel], dy[sel], dphi[sel], params_rows=rows[:, sel], **kw)
            assert s.last_flags == flag, name
            assert (one[3][3] == -1) == (flag != 0), name
            assert np.all(np.delete(one[3], 3) >= 0), name
        # the legal one is solved, as the polish solves it
        th = cr.expand(rows[:, [legal]], H, vv[[legal]], dy[[legal]], dphi[[legal]])
        u = np.zeros((2 * H, 1))
        _, pst, prin, prout = s.polish_batch_general(*[th[k] for k in NAMES], u, tol=TOL, max_rounds=ROUNDS, inputs=2)
    assert np.all(st[bad] == -1) and not bits(front[bad]).any() and not bits(rear[bad]).any()
    assert not bits(seq[:, bad]).any() and not bits(rin[bad]).any() and not bits(rout[bad]).any()
    assert st[legal] >= 0 and st[legal] == pst[0] and seq[:, legal].tobytes() == u[:, 0].tobytes()
    assert bits(rin[legal]) == bits(prin[0]) and bits(rout[legal]) == bits(prout[0])
    rest = np.setdiff1d(np.arange(N), at)
    assert np.array_equal(st[rest], clean["st"][rest]) and np.array_equal(bits(seq[:, rest]), bits(clean["seq"][:, rest]))
    assert np.array_equal(bits(front[rest]), bits(clean["front"][rest]))
    assert np.array_equal(bits(rin[rest]), bits(clean["rin"][rest]))
    assert int((st < 0).sum()) == int((clean["st"] < 0).sum()) + 6


# ---- backward

@functools.lru_cache(maxsize=None)
def _forward(H, recipe, n=NB):
    v, dy, dphi = compact_inputs(H, n)
    rows = cr.recipe_rows(recipe, H, n)
    with MpcSolver(horizon=H, device=None) as s:
        _, _, seq, st, _ = s.solve_batch_compact_exact(v, dy, dphi, tol=TOL, max_rounds=ROUNDS, fallback="none",
                                                       want_sequence=True, params_rows=rows)
    return v, dy, dphi, rows, seq, st


@pytest.mark.parametrize("with_sequence", [False, True])
@pytest.mark.parametrize("recipe", cr.RECIPES)
@pytest.mark.parametrize("H", HS)
def test_backward_equals_the_general_backward_through_the_chain_rule(H, recipe, with_sequence):
    v, dy, dphi, rows, seq, st = _forward(H, recipe)
    gf, gr, gs = cg.grad_in(H, NB, 11 + H, sequence=with_sequence)
    with MpcSolver(horizon=H, device=None) as s:
        ref, rflags = cr.reference(s, rows, H, v, dy, dphi, seq, gf, gr, gs)
        got = s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, gs, status=st, want=ALL, params_rows=rows)
        flags = s.last_flags
        free = s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, gs, status=None, want=ALL,
                                                    params_rows=rows)
        assert s.last_flags == 0 and flags == 0 and rflags == 0
    ok = st >= 0
    print(f"H={H} {recipe}: verified {int(ok.sum())}/{NB}")
    assert ok.any()
    for k in cg.PER_INSTANCE:
        assert cg.same_numbers(got[k][..., ok], ref[k][..., ok]), k          # the instances with status >= 0
        assert cg.same_numbers(free[k], ref[k]), k                           # status = NULL: every instance
        assert not bits(got[k][..., ~ok]).any(), k
    assert np.isfinite(got["params"]).all()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("H", [4, 5, 7, 20])
def test_backward_with_constant_rows_equals_the_shared_backward(H, variant):
    v, dy, dphi = compact_inputs(H, NB)
    gf, gr, gs = cg.grad_in(H, NB, 31 + H, sequence=True)
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        _, _, seq, st, _ = s.solve_batch_compact_exact(v, dy, dphi, tol=TOL, max_rounds=ROUNDS, fallback="none",
                                                       want_sequence=True)
        shared = s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, gs, status=st, want=ALL)
        rows = cr.shared_rows(s.params, NB)
    with MpcSolver(horizon=H, device=None) as s:
        got = s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, gs, status=st, want=ALL, params_rows=rows)
        assert s.last_flags == 0
    for k in ALL:                  # on the host-only handle both sum dparams in ascending k
        assert got[k].tobytes() == shared[k].tobytes(), k


def test_backward_excludes_invalid_instances():
    H = 10
    v, dy, dphi, rows, _, st0 = _forward(H, "all")
    at = _verified_seven(st0)
    rows, vv = cr.spoil(rows, v, at)
    bad = at[:6]
    gf, gr, gs = cg.grad_in(H, NB, 13, sequence=True)
    with MpcSolver(horizon=H, device=None) as s:
        _, _, seq, st, _ = s.solve_batch_compact_exact(vv, dy, dphi, tol=TOL, max_rounds=ROUNDS, fallback="none",
                                                       want_sequence=True, params_rows=rows)
        for status in (st, None):          # excluded by their own test, with and without the forward's status
            got = s.solve_batch_compact_exact_backward(vv, dy, dphi, seq, gf, gr, gs, status=status, want=ALL,
                                                       params_rows=rows)
            assert s.last_flags == capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL
            keep = np.setdiff1d(np.arange(NB), bad)
            part = s.solve_batch_compact_exact_backward(
                vv[keep], dy[keep], dphi[keep], np.ascontiguousarray(seq[:, keep]), gf[keep], gr[keep],
                np.ascontiguousarray(gs[:, keep]), status=None if status is None else st[keep], want=ALL,
                params_rows=np.ascontiguousarray(rows[:, keep]))
            assert s.last_flags == 0
            for k in cg.PER_INSTANCE:
                assert not bits(got[k][..., bad]).any(), k
                assert np.array_equal(bits(got[k][..., keep]), bits(part[k])), k
            assert got["params"].tobytes() == part["params"].tobytes()       # they add nothing to dparams
            assert np.any(got["params_rows"][:, at[6]] != 0.0)               # the infinite bound is differentiated


def _step(x):
    ax = np.abs(x)
    return np.where(ax > 0.1, 1e-6 * np.maximum(1.0, ax), 1e-4 * ax)


@pytest.mark.parametrize("H,recipe", [(4, "all"), (5, "weights"), (10, "all"), (20, "weights")])
def test_central_differences_of_the_rows_forward(H, recipe):
    n = 256
    v, dy, dphi = compact_inputs(H, n)
    rows = cr.recipe_rows(recipe, H, n)
    one = np.ones(n)
    with MpcSolver(horizon=H, device=None) as s:
        def solve(rows_):
            front, rear, seq, st, _ = s.solve_batch_compact_exact(v, dy, dphi, tol=1e-12, max_rounds=32,
                                                                  fallback="none", want_sequence=True, params_rows=rows_)
            u = seq.reshape(H, 2, n)
            act = np.concatenate([(u <= rows_[cr.LO]), (u >= rows_[cr.HI])]).reshape(-1, n)
            return front, rear, st >= 0, act, seq, st
        _, _, keep, act0, seq, st = solve(rows)
        got = {"front": s.solve_batch_compact_exact_backward(v, dy, dphi, seq, grad_front=one, status=st,
                                                             want=("params_rows",), params_rows=rows)["params_rows"],
               "rear": s.solve_batch_compact_exact_backward(v, dy, dphi, seq, grad_rear=one, status=st,
                                                            want=("params_rows",), params_rows=rows)["params_rows"]}
        keep = keep.copy()
        fd = {"front": np.empty((10, n)), "rear": np.empty((10, n))}
        for c in range(10):
            h = _step(rows[c])
            vals = []
            for sign in (1.0, -1.0):
                moved = rows.copy()
                moved[c] = rows[c] + sign * h
                front, rear, ok, act, _, _ = solve(moved)
                keep &= ok & np.all(act == act0, axis=0)
                vals.append((front, rear))
            fd["front"][c] = (vals[0][0] - vals[1][0]) / (2 * h)
            fd["rear"][c] = (vals[0][1] - vals[1][1]) / (2 * h)
    kept = int(keep.sum())
    print(f"H={H} {recipe}: kept {kept}/{n}")
    assert kept >= n // 2
    worst = 0.0
    for out in ("front", "rear"):
        for c, name in enumerate(COMPACT_PARAM_NAMES):
            mine, theirs = got[out][c][keep], fd[out][c][keep]
            if not np.any(mine):          # a bound nobody kept sits on: both sides are zero
                assert not np.any(theirs), (out, name)
                continue
            err = np.linalg.norm(theirs - mine) / np.linalg.norm(mine)
            print(f"  d{out}/d{name}: norm-wise relative error {err:.3e}")
            worst = max(worst, err)
            assert err <= 1e-5, (out, name, err)
    print(f"H={H} {recipe}: worst {worst:.3e}")


@pytest.mark.parametrize("n", [1, 2, 4096])
def test_dparams_is_the_sum_of_the_rows(n):
    H = 20
    v, dy, dphi, rows, seq, st = _forward(H, "all", n=n)
    gf, gr, gs = cg.grad_in(H, n, 3, sequence=True)
    with MpcSolver(horizon=H, device=None) as s:
        got = s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, gs, status=st, want=ALL, params_rows=rows)
    out = got["params_rows"]
    diff = np.abs(got["params"] - cg.fsum_rows(out))
    print(f"n={n}: max |dparams - fsum| / bound {np.max(diff / np.maximum(cg.fsum_bound(out), 1e-300)):.3f}")
    assert np.all(diff <= cg.fsum_bound(out)), (diff, cg.fsum_bound(out))
    acc = np.zeros(10)                     # the host-only handle sums in ascending k
    for k in range(n):
        acc = acc + out[:, k]
    assert np.array_equal(got["params"], acc)


# ---- the argument checks

def _raw(h, backward=False, n=3, H=4, q=True, g=True, tol=TOL, rounds=ROUNDS, fallback=capi.NEWTON_FALLBACK_NONE,
         mem=capi.HOST, dtype=capi.F64, null=None, **over):
    p = capi.default_params(H if 1 <= H <= 64 else 20, dtype=dtype, **over)
    p.horizon = H
    m = max(n, 1)
    v, dy, dphi = compact_inputs(4, m)
    rows = cr.shared_rows(capi.default_params(4), m)
    front, rear = np.full(m, 7.0), np.full(m, 7.0)
    ptr = lambda a, name: None if null == name else a.ctypes.data
    flags = C.c_uint32(99)
    lib = capi.load_library()
    if not backward:
        qq = capi.Polish(tol=tol, max_rounds=rounds)
        rc = lib.tpc_mpc_solve_batch_compact_exact_rows(
            h, C.byref(p), n, ptr(v, "v"), ptr(dy, "dy"), ptr(dphi, "dphi"), ptr(rows, "rows"),
            C.byref(qq) if q else None, fallback, ptr(front, "front"), ptr(rear, "rear"), None, None, C.byref(flags),
            mem, None)
        return rc, flags.value, front
    seq = np.zeros((2 * max(min(H, 64), 1), m))
    gf = np.ones(m)
    out = {"dv": front, "dparams": np.full(10, 7.0)}
    gg = capi.CompactGrad(grad_front=gf.ctypes.data, **{k: a.ctypes.data for k, a in out.items()})
    rc = lib.tpc_mpc_solve_batch_compact_exact_rows_backward(
        h, C.byref(p), n, ptr(v, "v"), ptr(dy, "dy"), ptr(dphi, "dphi"), ptr(rows, "rows"), ptr(seq, "sequence"), None,
        C.byref(gg) if g else None, C.byref(flags), mem, None)
    return rc, flags.value, out


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


BAD_ARG, BAD_HORIZON, BAD_EPS, NO_DEVICE = 1, 4, 5, 6
# p's ten model fields are neither read nor validated
IGNORED = (dict(weight_y=-1.0), dict(weight_steering_rear=0.0), dict(weight_phi=np.nan), dict(step_size=np.inf),
           dict(wheelbase=0.0), dict(lower=(0.1, -0.1), upper=(0.0, 0.1)))


def test_forward_degenerate_calls_and_argument_errors(host_handle):
    h = host_handle
    rc, flags, front = _raw(h)                      # the plain call, every optional output NULL
    assert (rc, flags) == (0, 0) and np.all(front != 7.0)
    rc, flags, front = _raw(h, n=0)
    assert (rc, flags) == (0, 0) and np.all(front == 7.0)
    assert _raw(h, n=0, null="rows")[:2] == (0, 0)      # n == 0 returns before the batch pointers are looked at
    for kw in (dict(q=False), dict(tol=0.0), dict(tol=-1e-9), dict(tol=np.nan), dict(rounds=-1), dict(fallback=2),
               dict(fallback=-1), dict(dtype=capi.F32), dict(n=-1), dict(mem=5), dict(null="v"), dict(null="dy"),
               dict(null="dphi"), dict(null="front"), dict(null="rear"), dict(null="rows")):
        assert _raw(h, **kw)[0] == BAD_ARG, kw
    assert _raw(h, null="rows")[0] == BAD_ARG and b"params_rows" in capi.load_library().tpc_mpc_last_error(h)
    assert _raw(h, dtype=capi.F32)[0] == BAD_ARG and b"fp64" in capi.load_library().tpc_mpc_last_error(h)
    for kw in IGNORED:
        rc, flags, got = _raw(h, **kw)
        assert (rc, flags) == (0, 0) and got.tobytes() == _raw(h)[2].tobytes(), kw
    assert _raw(h, H=65)[0] == BAD_HORIZON and _raw(h, H=0)[0] == BAD_HORIZON
    assert _raw(h, eps=0.0)[0] == BAD_EPS
    # a host-only handle: no fallback solve and no DEVICE memory -- reported after the argument checks
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE)[0] == NO_DEVICE
    assert _raw(h, mem=capi.DEVICE)[0] == NO_DEVICE
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE, tol=0.0)[0] == BAD_ARG
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE, n=0)[0] == NO_DEVICE
    with MpcSolver(horizon=4, device=None) as s:
        v, dy, dphi = compact_inputs(4, 8)
        with pytest.raises(capi.TpcMpcError) as e:
            s.solve_batch_compact_exact(v, dy, dphi, params_rows=cr.shared_rows(s.params, 8))    # fallback="solve"
        assert e.value.status == NO_DEVICE
        with pytest.raises(ValueError):
            s.solve_batch_compact_exact(v, dy, dphi, fallback="none", params_rows=np.zeros((10, 7)))


def test_backward_degenerate_calls_and_argument_errors(host_handle):
    h = host_handle
    rc, flags, out = _raw(h, backward=True)
    assert (rc, flags) == (0, 0) and np.all(out["dv"] != 7.0) and np.all(out["dparams"] != 7.0)
    rc, flags, out = _raw(h, backward=True, n=0)      # n == 0: OK, flags 0, zeros in dparams, nothing else touched
    assert (rc, flags) == (0, 0) and not bits(out["dparams"]).any() and np.all(out["dv"] == 7.0)
    for kw in (dict(g=False), dict(null="sequence"), dict(dtype=capi.F32), dict(n=-1), dict(mem=5), dict(null="v"),
               dict(null="dy"), dict(null="dphi"), dict(null="rows")):
        assert _raw(h, backward=True, **kw)[0] == BAD_ARG, kw
    assert _raw(h, backward=True, null="rows")[0] == BAD_ARG
    assert b"params_rows" in capi.load_library().tpc_mpc_last_error(h)
    base = _raw(h, backward=True)[2]
    for kw in IGNORED:
        rc, flags, got = _raw(h, backward=True, **kw)
        assert (rc, flags) == (0, 0), kw
        assert all(got[k].tobytes() == base[k].tobytes() for k in got), kw
    assert _raw(h, backward=True, H=65)[0] == BAD_HORIZON and _raw(h, backward=True, eps=0.0)[0] == BAD_EPS
    assert _raw(h, backward=True, mem=capi.DEVICE)[0] == NO_DEVICE
    assert _raw(h, backward=True, mem=capi.DEVICE, g=False)[0] == BAD_ARG       # reported after the argument checks
    with MpcSolver(horizon=4, device=None) as s:
        with pytest.raises(ValueError):
            s.solve_batch_compact_exact_backward(*compact_inputs(4, 8), np.zeros((8, 8)), params_rows=np.zeros((10, 7)))


def test_symbols_are_declared_and_documented():
    lib = capi.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tpc_mpc.h")) as f:
        text = f.read()
    for name in ("tpc_mpc_solve_batch_compact_exact_rows", "tpc_mpc_solve_batch_compact_exact_rows_backward"):
        assert name in capi.EXPORTS and hasattr(lib, name) and f"int {name}(" in text
    assert "#define TPC_MPC_ABI_VERSION 5 " in text
