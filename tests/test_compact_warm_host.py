"""CPU tests of the warm-started exact compact solve (tpc_mpc_solve_batch_compact_exact_from,
MpcSolver.solve_batch_compact_exact(start=...)) on a host-only handle, which runs the kernels' arithmetic on the calling
thread with TPC_MPC_NEWTON_FALLBACK_NONE.

The bits against tpc_mpc_polish_batch_general(controls = start) on the expanded arrays for three kinds of start; a start
of zeros and a start with a NaN / Inf against the cold entry; sequence_out == start; the share a warm start verifies and
how far a warm answer lies from the cold one, as conditions; invalid columns, n == 0, the argument checks.

Batch.  n = 4096 instances of compact_inputs(H, 4096), tol 1e-9, 16 rounds, as the parents' tests.  "moved" starts: the
model's own cold answers (zeros where the cold start does not verify), then the four weights moved by 1 % (+, -, +, -)
-- one step of a fitting loop.

Coverage (test_coverage_from_the_previous_optimum).  The starts are each instance's optimum at the default weights,
cold, with 64 rounds.  Among the instances that have such a start the unverified after a 1 % move, measured with
tpc_mpc_polish_batch_general(controls = start) before the entry existed: 0 of 4058 (H = 10), 0 of 3999 (H = 20), 4 of
3958 = 0.10 % (H = 40), at 1.07 / 1.15 / 1.28 mean rounds against 2.51 / 2.64 / 2.64 cold.  The condition is 0.5 %.

Warm against cold (test_warm_answers_equal_cold_answers).  Both stop at a point whose residual is <= tol, not at the
same point: the largest |warm - cold| over the instances both verify was measured against the cold entry at 1.1e-14 /
1.3e-13 / 1.4e-12 (H = 10 / 20 / 40) and is asserted at 10x that."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests.model import compact_rows_common as cr
from tests.model import compact_warm_common as cw
from tests.model.compact_exact_common import N, ROUNDS, TOL, VARIANTS, bits
from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd.synth import compact_inputs

HS = (1, 4, 5, 7, 10, 20, 40, 64)
MODELS = ([("shared", "default", H) for H in HS]
          + [("shared", name, H) for name in VARIANTS if name != "default" for H in (4, 5, 7, 20)]
          + [("rows", recipe, H) for recipe in cr.RECIPES for H in HS])
MOVE = 0.01
COVERAGE_HS = (10, 20, 40)
COVERAGE_SHARE = 0.005
WARM_COLD_MEASURED = {10: 1.1e-14, 20: 1.3e-13, 40: 1.4e-12}


def _same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _cold(kind, name, H):
    """the cold entry on the case's model and on the model moved by one step, shared by the tests (never modified)"""
    v, dy, dphi = compact_inputs(H, N)
    with MpcSolver(horizon=H, device=None) as s:
        base = cw.solve(s, cw.model(kind, name, H, N), v, dy, dphi)
        moved = cw.solve(s, cw.model(kind, name, H, N, MOVE), v, dy, dphi)
        flags = s.last_flags
    return base, moved, flags


def _start(kind, name, H, which):
    if which == "moved":
        return _cold(kind, name, H)[0][2]
    if which == "random":
        return cw.random_start(H, N, 77 + H)
    return np.zeros((2 * H, N))


@functools.lru_cache(maxsize=None)
def _warm(kind, name, H, which):
    v, dy, dphi = compact_inputs(H, N)
    m = cw.model(kind, name, H, N, MOVE)
    start = _start(kind, name, H, which)
    with MpcSolver(horizon=H, device=None) as s:
        got = cw.solve(s, m, v, dy, dphi, start=start)
        flags = s.last_flags
        ref = cw.polish(s, m, H, v, dy, dphi, start)
        pflags = s.last_flags
    return got, flags, ref, pflags


# ---- against the polish

@pytest.mark.parametrize("which", cw.STARTS)
@pytest.mark.parametrize("kind,name,H", MODELS)
def test_bits_equal_the_polish_from_the_same_start(kind, name, H, which):
    (front, rear, seq, st, fb, rin, rout), flags, (pu, pst, prin, prout), pflags = _warm(kind, name, H, which)
    ok = st >= 0
    print(f"{kind} {name} H={H} {which}: verified {int(ok.sum())}/{N}, mean rounds "
          f"{st[ok].mean() if ok.any() else 0:.3f}")
    assert fb is None
    assert np.array_equal(st, pst)
    assert np.array_equal(bits(rin), bits(prin))
    assert np.array_equal(bits(rout[ok]), bits(prout[ok])) and not bits(rout[~ok]).any()
    assert np.array_equal(bits(seq[:, ok]), bits(pu[:, ok]))          # signed zeros included
    assert np.array_equal(bits(front[ok]), bits(pu[0, ok])) and np.array_equal(bits(rear[ok]), bits(pu[1, ok]))
    # unverified: zeros, as the parents return them
    assert not bits(seq[:, ~ok]).any() and not bits(front[~ok]).any() and not bits(rear[~ok]).any()
    assert flags == pflags
    if which == "random":                                              # the start reaches outside every box
        assert np.abs(_start(kind, name, H, which)).max() > cr.AMAX


@pytest.mark.parametrize("kind,name,H", MODELS)
def test_a_start_of_zeros_is_the_cold_entry(kind, name, H):
    got, flags, _, _ = _warm(kind, name, H, "zeros")
    _, cold, cflags = _cold(kind, name, H)
    assert _same(got, cold) and flags == cflags


# ---- no start

@pytest.mark.parametrize("kind,name,H", [("shared", "default", 4), ("shared", "offset", 5), ("shared", "default", 20),
                                         ("rows", "all", 5), ("rows", "all", 7), ("rows", "weights", 40)])
def test_a_nonfinite_column_is_that_instance_of_the_cold_entry(kind, name, H):
    warm, wflags, _, _ = _warm(kind, name, H, "moved")
    _, cold, _ = _cold(kind, name, H)
    start = _start(kind, name, H, "moved").copy()
    rng = np.random.default_rng(5 + H)
    none = np.sort(rng.choice(N, 300, replace=False))
    # one component each: the first, the last, any; NaN, +Inf, -Inf
    comp = np.where(np.arange(300) % 3 == 0, 0, np.where(np.arange(300) % 3 == 1, 2 * H - 1, rng.integers(0, 2 * H, 300)))
    start[comp, none] = np.array([np.nan, np.inf, -np.inf])[rng.integers(0, 3, 300)]
    v, dy, dphi = compact_inputs(H, N)
    with MpcSolver(horizon=H, device=None) as s:
        got = cw.solve(s, cw.model(kind, name, H, N, MOVE), v, dy, dphi, start=start)
        flags = s.last_flags
    rest = np.setdiff1d(np.arange(N), none)
    for g, c, w in zip(got, cold, warm):
        if g is None:
            continue
        assert g[..., none].tobytes() == c[..., none].tobytes()        # the cold entry's bits
        assert g[..., rest].tobytes() == w[..., rest].tobytes()        # the neighbours are untouched
    # no flag of their own: NOT_POLISHED exactly when somebody is left unverified
    assert flags == (capi.FLAG_NOT_POLISHED if np.any(got[3] < 0) else 0)
    assert not flags & capi.FLAG_NONFINITE
    assert np.any(cold[3][none] >= 0)


# ---- in place

@pytest.mark.parametrize("kind,name,H", [("shared", "default", 1), ("shared", "default", 4), ("shared", "asymmetric", 5),
                                         ("shared", "default", 20), ("rows", "all", 4), ("rows", "all", 10),
                                         ("rows", "weights", 64)])
def test_sequence_out_may_be_the_start(kind, name, H):
    warm, wflags, _, _ = _warm(kind, name, H, "moved")
    v, dy, dphi = compact_inputs(H, N)
    m = cw.model(kind, name, H, N, MOVE)
    start = _start(kind, name, H, "moved").copy()
    start[0, 17] = np.nan                                              # and an instance with no start among them
    lib = capi.load_library()
    with MpcSolver(horizon=H, device=None) as s:
        p = s._params(**m["over"])
        out = cw.raw_from(lib, s._h, p, v, dy, dphi, start.copy(), rows=m["rows"])
        inp = cw.raw_from(lib, s._h, p, v, dy, dphi, start, rows=m["rows"], in_place=True)
    assert out[0] == 0 and inp[0] == 0 and out[1] == inp[1]
    assert inp[4] is start
    for a, b in zip(out[2:], inp[2:]):
        assert a.tobytes() == b.tobytes()
    keep = np.setdiff1d(np.arange(N), [17])
    assert out[4][:, keep].tobytes() == warm[2][:, keep].tobytes() and np.array_equal(out[5][keep], warm[3][keep])


# ---- coverage and the distance to the cold answer, as conditions

@functools.lru_cache(maxsize=None)
def _previous_optimum(H):
    """each instance's optimum at the default weights, cold, with a large round cap; `have`: who has one"""
    v, dy, dphi = compact_inputs(H, N)
    with MpcSolver(horizon=H, device=None) as s:
        out = cw.solve(s, cw.model("shared", "default", H, N), v, dy, dphi, rounds=64)
    return out[2], out[3] >= 0


@pytest.mark.parametrize("H", COVERAGE_HS)
def test_coverage_from_the_previous_optimum(H):
    start, have = _previous_optimum(H)
    v, dy, dphi = compact_inputs(H, N)
    with MpcSolver(horizon=H, device=None) as s:
        warm = cw.solve(s, cw.model("shared", "default", H, N, MOVE), v, dy, dphi, start=start)
    cold = _cold("shared", "default", H)[1]
    wst, cst = warm[3], cold[3]
    left = int((wst[have] < 0).sum())
    print(f"H={H}: {int(have.sum())} instances have a start; unverified among them warm {left} "
          f"({100.0 * left / have.sum():.2f} %), cold {int((cst[have] < 0).sum())}; whole batch cold "
          f"{int((cst < 0).sum())}; mean rounds warm {wst[have & (wst >= 0)].mean():.2f}, cold {cst[cst >= 0].mean():.2f}; "
          f"warm rounds histogram {np.bincount(wst[have & (wst >= 0)]).tolist()}")
    assert have.sum() >= 0.9 * N
    assert left <= COVERAGE_SHARE * have.sum()


@pytest.mark.parametrize("H", COVERAGE_HS)
def test_warm_answers_equal_cold_answers(H):
    start, have = _previous_optimum(H)
    v, dy, dphi = compact_inputs(H, N)
    with MpcSolver(horizon=H, device=None) as s:
        warm = cw.solve(s, cw.model("shared", "default", H, N, MOVE), v, dy, dphi, start=start)
    cold = _cold("shared", "default", H)[1]
    both = (warm[3] >= 0) & (cold[3] >= 0)
    worst = float(np.abs(warm[2][:, both] - cold[2][:, both]).max())
    print(f"H={H}: both verify {int(both.sum())}/{N}, max |warm - cold| {worst:.3e} "
          f"(measured {WARM_COLD_MEASURED[H]:.1e}, bound 10x)")
    assert both.sum() >= 0.9 * N
    assert worst <= 10 * WARM_COLD_MEASURED[H]


# ---- the rest: invalid columns, n == 0, the argument checks

@pytest.mark.parametrize("H", [4, 20])
def test_invalid_rows_columns_with_a_start(H):
    base, _, _ = _cold("rows", "all", H)
    clean, cflags, _, _ = _warm("rows", "all", H, "moved")
    v, dy, dphi = compact_inputs(H, N)
    m = cw.model("rows", "all", H, N, MOVE)
    at = np.flatnonzero((clean[3] >= 0) & (base[3] >= 0))[[3, 40, 100, 150, 200, 300, 400]]
    rows, vv = cr.spoil(m["rows"], v, at)
    bad, legal = at[:6], at[6]
    start = base[2]
    with MpcSolver(horizon=H, device=None) as s:
        front, rear, seq, st, _, rin, rout = cw.solve(s, dict(over={}, rows=rows), vv, dy, dphi, start=start)
        # no NOT_POLISHED of their own: only what the clean batch raises
        assert s.last_flags == capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL | cflags
        one = [legal]
        pu, pst, prin, prout = cw.polish(s, dict(over={}, rows=rows[:, one]), H, vv[one], dy[one], dphi[one],
                                         start[:, one])
    assert np.all(st[bad] == -1) and not bits(front[bad]).any() and not bits(rear[bad]).any()
    assert not bits(seq[:, bad]).any() and not bits(rin[bad]).any() and not bits(rout[bad]).any()
    # the legal one (an infinite bound) is solved from its start, as the polish solves it
    assert st[legal] >= 0 and st[legal] == pst[0] and seq[:, legal].tobytes() == pu[:, 0].tobytes()
    assert bits(rin[legal]) == bits(prin[0]) and bits(rout[legal]) == bits(prout[0])
    rest = np.setdiff1d(np.arange(N), at)
    for g, c in zip((front, rear, seq, st, rin, rout), (clean[0], clean[1], clean[2], clean[3], clean[5], clean[6])):
        assert g[..., rest].tobytes() == c[..., rest].tobytes()


def _raw(h, n=3, H=4, q=True, tol=TOL, rounds=ROUNDS, fallback=capi.NEWTON_FALLBACK_NONE, mem=capi.HOST,
         dtype=capi.F64, null=None, rows=False, **over):
    p = capi.default_params(H if 1 <= H <= 64 else 20, dtype=dtype, **over)
    p.horizon = H
    m = max(n, 1)
    v, dy, dphi = compact_inputs(4, m)
    prow = cr.shared_rows(capi.default_params(4), m)
    start = np.full((2 * max(min(H, 64), 1), m), 0.01)
    front, rear = np.full(m, 7.0), np.full(m, 7.0)
    ptr = lambda a, name: None if null == name else a.ctypes.data
    flags = C.c_uint32(99)
    qq = capi.Polish(tol=tol, max_rounds=rounds)
    rc = capi.load_library().tpc_mpc_solve_batch_compact_exact_from(
        h, C.byref(p), n, ptr(v, "v"), ptr(dy, "dy"), ptr(dphi, "dphi"), ptr(prow, "rows") if rows else None,
        ptr(start, "start"), C.byref(qq) if q else None, fallback, ptr(front, "front"), ptr(rear, "rear"), None, None,
        C.byref(flags), mem, None)
    return rc, flags.value, front


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


BAD_ARG, BAD_HORIZON, BAD_EPS, NO_DEVICE = 1, 4, 5, 6
# the shared entry validates p's model as tpc_mpc_solve_batch_compact does; with params_rows they are not read
MODEL_ERRORS = (dict(weight_y=-1.0), dict(weight_steering_rear=0.0), dict(weight_phi=np.nan), dict(step_size=np.inf),
                dict(wheelbase=0.0), dict(lower=(0.1, -0.1), upper=(0.0, 0.1)))


@pytest.mark.parametrize("rows", [False, True])
def test_degenerate_calls_and_argument_errors(host_handle, rows):
    h = host_handle
    lib = capi.load_library()
    rc, flags, front = _raw(h, rows=rows)                 # the plain call, every optional output NULL
    assert (rc, flags) == (0, 0) and np.all(front != 7.0)
    rc, flags, front = _raw(h, n=0, rows=rows)
    assert (rc, flags) == (0, 0) and np.all(front == 7.0)
    assert _raw(h, n=0, null="start", rows=rows)[:2] == (0, 0)   # n == 0 returns before the batch pointers are looked at
    for kw in (dict(q=False), dict(tol=0.0), dict(tol=-1e-9), dict(tol=np.nan), dict(rounds=-1), dict(fallback=2),
               dict(fallback=-1), dict(dtype=capi.F32), dict(n=-1), dict(mem=5), dict(null="v"), dict(null="dy"),
               dict(null="dphi"), dict(null="front"), dict(null="rear"), dict(null="start")):
        assert _raw(h, rows=rows, **kw)[0] == BAD_ARG, kw
    assert _raw(h, null="start", rows=rows)[0] == BAD_ARG and b"start" in lib.tpc_mpc_last_error(h)
    assert _raw(h, dtype=capi.F32, rows=rows)[0] == BAD_ARG and b"fp64" in lib.tpc_mpc_last_error(h)
    assert _raw(h, H=65, rows=rows)[0] == BAD_HORIZON and _raw(h, H=0, rows=rows)[0] == BAD_HORIZON
    assert _raw(h, eps=0.0, rows=rows)[0] == BAD_EPS
    for kw in MODEL_ERRORS:
        rc, flags, got = _raw(h, rows=rows, **kw)
        if rows:                                          # neither read nor validated
            assert (rc, flags) == (0, 0) and got.tobytes() == _raw(h, rows=True)[2].tobytes(), kw
        else:                                             # the cold shared entry's verdict, whatever it is
            p = capi.default_params(4, **kw)
            v, dy, dphi = compact_inputs(4, 3)
            out = np.empty(3)
            qq = capi.Polish(tol=TOL, max_rounds=ROUNDS)
            want = lib.tpc_mpc_solve_batch_compact_exact(h, C.byref(p), 3, v.ctypes.data, dy.ctypes.data,
                                                         dphi.ctypes.data, C.byref(qq), capi.NEWTON_FALLBACK_NONE,
                                                         out.ctypes.data, out.ctypes.data, None, None, None, capi.HOST,
                                                         None)
            assert rc == want and want != 0, kw
    # a host-only handle: no fallback solve and no DEVICE memory -- reported after the argument checks
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE, rows=rows)[0] == NO_DEVICE
    assert _raw(h, mem=capi.DEVICE, rows=rows)[0] == NO_DEVICE
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE, tol=0.0, rows=rows)[0] == BAD_ARG
    assert _raw(h, fallback=capi.NEWTON_FALLBACK_SOLVE, n=0, rows=rows)[0] == NO_DEVICE


def test_the_binding_checks_the_start():
    with MpcSolver(horizon=4, device=None) as s:
        v, dy, dphi = compact_inputs(4, 8)
        with pytest.raises(capi.TpcMpcError) as e:
            s.solve_batch_compact_exact(v, dy, dphi, start=np.zeros((8, 8)))          # fallback="solve"
        assert e.value.status == NO_DEVICE
        with pytest.raises(ValueError):
            s.solve_batch_compact_exact(v, dy, dphi, fallback="none", start=np.zeros((8, 7)))
        with pytest.raises(ValueError):
            s.solve_batch_compact_exact(v, dy, dphi, fallback="none", start=np.zeros((10, 8)))
        cold = s.solve_batch_compact_exact(v, dy, dphi, fallback="none", want_sequence=True)
        none = s.solve_batch_compact_exact(v, dy, dphi, fallback="none", want_sequence=True, start=None)
        assert _same(cold, none)


def test_the_symbol_is_declared_and_documented():
    lib = capi.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tpc_mpc.h")) as f:
        text = f.read()
    name = "tpc_mpc_solve_batch_compact_exact_from"
    assert name in capi.EXPORTS and hasattr(lib, name) and f"int {name}(" in text
    assert "#define TPC_MPC_ABI_VERSION 5 " in text
