"""CPU tests of the exact compact solve's forward mode (tpc_mpc_solve_batch_compact_exact_forward,
MpcSolver.solve_batch_compact_exact_forward) on a host-only handle, which runs the kernel's per-lane arithmetic on the
calling thread: the numbers against tpc_mpc_solve_batch_general_forward on the expanded arrays and tangents
(tests/model/compact_tangent_common.py), shared and per-instance parameters, the directions one by one, the transpose
identity against the backward pass, central differences of the exact forward, the excluded instances and the argument
checks.

Transpose identity.  <(gf, gr, gs), (tfront, trear, tsequence)> = <(dv, ddy, ddphi, dparams_rows), the direction> per
instance, in exact arithmetic for ANY sequence; mismatch() (tests/test_rollout_tangent_host.py) is relative to the sum
of the absolute values of every product.  The yardstick is the same identity through the general entries
(solve_batch_general_forward against solve_batch_general_backward) on the expanded arrays and tangents of the same
cases -- H in (4, 10, 20, 64), shared and per-instance parameters, n = 40, K = 2 -- measured on the CPU:
  general entries, largest mismatch   7.398e-12  (H = 64, per-instance parameters; 8e-16 .. 1.5e-13 at H <= 20)
  compact entries, largest mismatch   9.252e-12  (the same case; 1.2e-15 .. 3.6e-13 at H <= 20)
The bound is 10x the general entries' value, the project's convention; both grow with the horizon as the closed
loop's do (tests/test_rollout_tangent_host.py).  The compact chain rule adds six rounded operations and stays within
the bound.

Finite differences: the steps and the keep rule of tests/test_compact_grad_host.py, front and rear separately."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests.model import compact_rows_common as cr
from tests.model import compact_tangent_common as ct
from tests.model.compact_tangent_common import NAMES, VARIANTS, bits
from tests.test_compact_grad_host import FD_CASES, _forward, _step
from tests.test_rollout_tangent_host import mismatch
from trajectory_controller_amd import COMPACT_PARAM_NAMES, MpcSolver, capi
from trajectory_controller_amd.synth import compact_inputs

HS = (1, 4, 5, 7, 10, 20, 40, 64)
N, K = 512, 3
ALL = ("v", "delta_y", "delta_phi", "params", "params_rows", "kkt_residual")
GENERAL_MEASURED = 7.398e-12
BOUND = 10 * GENERAL_MEASURED


@functools.lru_cache(maxsize=None)
def _forward_rows(H, recipe, n=N):
    """the exact forward with per-instance parameters on the host-only handle, shared by the tests (never modified)"""
    v, dy, dphi = compact_inputs(H, n)
    rows = cr.recipe_rows(recipe, H, n)
    with MpcSolver(horizon=H, device=None) as s:
        _, _, seq, st, _ = s.solve_batch_compact_exact(v, dy, dphi, fallback="none", want_sequence=True, params_rows=rows)
    return v, dy, dphi, rows, seq, st


def _call(s, v, dy, dphi, seq, d, want_sequence, **kw):
    out = s.solve_batch_compact_exact_forward(v, dy, dphi, seq, d, want_sequence=want_sequence, **kw)
    return out, s.last_flags


def _check_against(ref, got, free, st, want_sequence):
    ok = st >= 0
    assert ok.any()
    assert ct.same_numbers(got[0][:, ok], ref[:, 0][:, ok]) and ct.same_numbers(got[1][:, ok], ref[:, 1][:, ok])
    assert ct.same_numbers(free[0], ref[:, 0]) and ct.same_numbers(free[1], ref[:, 1])   # status=None: every instance
    for a in got:
        assert not np.any(a[..., ~ok])                               # excluded columns are all zero
    if want_sequence:
        assert ct.same_numbers(got[2][..., ok], ref[..., ok]) and ct.same_numbers(free[2], ref)
        assert ct.same_numbers(got[2][:, 0], got[0]) and ct.same_numbers(got[2][:, 1], got[1])   # row 0
    assert np.abs(ref[:, 0]).max() > 0 and np.abs(ref[:, 1]).max() > 0


@pytest.mark.parametrize("want_sequence", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("H", HS)
def test_numbers_equal_the_general_forward_on_the_expanded_tangents(H, variant, want_sequence):
    v, dy, dphi, seq, st, _, _ = _forward(H, variant)
    d = ct.directions(N, K, 31 + H)
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        p = s.params
        ref, rflags = ct.reference(s, ct.expand(p, H, v, dy, dphi), p.step_size, p.wheelbase, H, v, seq, d, K)
        got, flags = _call(s, v, dy, dphi, seq, d, want_sequence, status=st)
        free, fflags = _call(s, v, dy, dphi, seq, d, want_sequence)
        assert (rflags, flags, fflags) == (0, 0, 0)
        # constant rows, with "params_rows" constant along n, give the shared call's bytes
        rows = cr.shared_rows(p, N)
        dr = {k: a for k, a in d.items() if k != "params"}
        dr["params_rows"] = ct.params_tangent(d, K, N)
        same, sflags = _call(s, v, dy, dphi, seq, dr, want_sequence, status=st, params_rows=rows)
        assert sflags == 0
    print(f"H={H} {variant}: verified {int((st >= 0).sum())}/{N}")
    _check_against(ref, got, free, st, want_sequence)
    for a, b in zip(same, got):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("want_sequence", [False, True])
@pytest.mark.parametrize("recipe", cr.RECIPES)
@pytest.mark.parametrize("H", HS)
def test_rows_numbers_equal_the_general_forward(H, recipe, want_sequence):
    v, dy, dphi, rows, seq, st = _forward_rows(H, recipe)
    d = ct.directions(N, K, 57 + H, rows=True)
    with MpcSolver(horizon=H, device=None) as s:
        ref, rflags = ct.reference(s, cr.expand(rows, H, v, dy, dphi), rows[ct.T], rows[ct.L], H, v, seq, d, K)
        got, flags = _call(s, v, dy, dphi, seq, d, want_sequence, status=st, params_rows=rows)
        free, fflags = _call(s, v, dy, dphi, seq, d, want_sequence, params_rows=rows)
        assert (rflags, flags, fflags) == (0, 0, 0)
    _check_against(ref, got, free, st, want_sequence)


@pytest.mark.parametrize("H", (4, 7, 20))
def test_directions_are_independent_and_a_missing_key_is_zero(H):
    v, dy, dphi, seq, st, _, _ = _forward(H, "asymmetric")
    _, _, _, rows, rseq, rst = _forward_rows(H, "all")
    with MpcSolver(horizon=H, device=None, **VARIANTS["asymmetric"]) as s:
        for shared in (True, False):
            d = ct.directions(N, K, 3 + H, rows=not shared)
            kw = dict(status=st) if shared else dict(status=rst, params_rows=rows)
            sq = seq if shared else rseq
            full, _ = _call(s, v, dy, dphi, sq, d, True, **kw)
            for i in range(K):
                one, flags = _call(s, v, dy, dphi, sq, {k: np.ascontiguousarray(a[i]) for k, a in d.items()}, True, **kw)
                assert flags == 0
                for a, b in zip(full, one):
                    assert b.shape[0] == 1 and np.array_equal(bits(a[i]), bits(b[0]))
            for missing in d:
                part = {k: a for k, a in d.items() if k != missing}
                zeros = dict(part)
                zeros[missing] = np.zeros_like(d[missing])
                a, _ = _call(s, v, dy, dphi, sq, part, True, **kw)
                b, _ = _call(s, v, dy, dphi, sq, zeros, True, **kw)
                for x, y in zip(a, b):
                    assert np.array_equal(bits(x), bits(y)), missing
                assert not np.array_equal(bits(a[0]), bits(full[0])), missing


def _identity(s, H, n, shared, seed=0):
    """(compact mismatch, general mismatch) [K, n] of the transpose identity on one case"""
    K2 = 2
    if shared:
        v, dy, dphi, seq, _, _, _ = _forward(H, "default", n=n)
        rows, p = None, s.params
        th, T_, l_ = ct.expand(p, H, v, dy, dphi), p.step_size, p.wheelbase
    else:
        v, dy, dphi, rows, seq, _ = _forward_rows(H, "all", n=n)
        th, T_, l_ = cr.expand(rows, H, v, dy, dphi), rows[ct.T], rows[ct.L]
    rng = np.random.default_rng(5 + seed + H)
    gf, gr, gs = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal((2 * H, n))
    d = ct.directions(n, K2, 9 + seed + H, rows=not shared)
    kw = {} if shared else dict(params_rows=rows)
    tf, tr, ts = s.solve_batch_compact_exact_forward(v, dy, dphi, seq, d, want_sequence=True, **kw)
    assert s.last_flags == 0
    g = s.solve_batch_compact_exact_backward(v, dy, dphi, seq, gf, gr, gs, want=ALL, **kw)
    assert s.last_flags == 0
    tp = ct.params_tangent(d, K2, n)
    compact = np.stack([mismatch([gf[None] * tf[i][None], gr[None] * tr[i][None], gs * ts[i]],
                                 [g["v"][None] * d["v"][i][None], g["delta_y"][None] * d["delta_y"][i][None],
                                  g["delta_phi"][None] * d["delta_phi"][i][None], g["params_rows"] * tp[i]])
                        for i in range(K2)])
    # the yardstick: the same identity through the general entries on the expanded arrays and tangents
    G = rng.standard_normal((2 * H, n))
    tan = ct.expand_tangents(T_, l_, H, v, d, K2)
    ins = [th[k] for k in NAMES]
    tu = s.solve_batch_general_forward(*ins, seq, tan, inputs=2)
    assert s.last_flags == 0
    gg = s.solve_batch_general_backward(*ins, seq, G, inputs=2)
    assert s.last_flags == 0
    general = np.stack([mismatch([G * tu[i]], [gg[k] * tan[k][i] for k in tan]) for i in range(K2)])
    return compact, general


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("H", (4, 10, 20, 64))
def test_transpose_identity_against_the_backward(H, shared):
    with MpcSolver(horizon=H, device=None) as s:
        compact, general = _identity(s, H, 40, shared)
    print(f"H={H} {'shared' if shared else 'rows'}: compact {compact.max():.3e} general {general.max():.3e} "
          f"bound {BOUND:.3e}")
    assert general.max() <= GENERAL_MEASURED * 1.0001          # the yardstick is what the header says
    assert compact.max() > 0.0
    assert compact.max() <= BOUND


@pytest.mark.parametrize("H,variant", FD_CASES)
def test_finite_differences_of_the_exact_forward(H, variant):
    n = 256
    v, dy, dphi = compact_inputs(H, n)
    names = COMPACT_PARAM_NAMES[:6]
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        p0 = s.params
        lo, hi = np.array(p0.lower)[:, None], np.array(p0.upper)[:, None]

        def solve(v_, dy_, dphi_, **over):
            front, rear, seq, st, _ = s.solve_batch_compact_exact(v_, dy_, dphi_, tol=1e-12, max_rounds=32,
                                                                  fallback="none", want_sequence=True, **over)
            u = seq.reshape(H, 2, n)
            act = np.concatenate([(u <= lo), (u >= hi)]).reshape(-1, n)
            return (front, rear), st >= 0, act, seq, st
        _, ok0, act0, seq, st = solve(v, dy, dphi)
        # K = 9 unit directions: v, delta_y, delta_phi, and the first six parameters through "params"
        d = {k: np.zeros((9, n)) for k in ct.VECTORS}
        for i, k in enumerate(ct.VECTORS):
            d[k][i] = 1.0
        d["params"] = np.zeros((9, 10))
        for c in range(6):
            d["params"][3 + c, c] = 1.0
        tf, tr = s.solve_batch_compact_exact_forward(v, dy, dphi, seq, d, status=st)
        assert s.last_flags == 0
        keep = ok0.copy()
        fd = {}

        def central(key, lo_args, hi_args, h):
            nonlocal keep
            vals = []
            for args, over in (hi_args, lo_args):
                out, ok, act, _, _ = solve(*args, **over)
                keep &= ok & np.all(act == act0, axis=0)
                vals.append(out)
            fd[key] = [(vals[0][j] - vals[1][j]) / (2 * h) for j in range(2)]
        ins = dict(v=v, delta_y=dy, delta_phi=dphi)
        for key in ins:
            h = _step(ins[key]) * np.sign(ins[key])
            plus = [ins[k] + h if k == key else ins[k] for k in ins]
            minus = [ins[k] - h if k == key else ins[k] for k in ins]
            central(key, (minus, {}), (plus, {}), h)
        for c, name in enumerate(names):
            x = getattr(p0, name)
            h = float(_step(np.float64(x)))
            central(name, ((v, dy, dphi), {name: x - h}), ((v, dy, dphi), {name: x + h}), h)
    kept = int(keep.sum())
    print(f"H={H} {variant}: kept {kept}/{n}")
    assert kept >= 200
    worst = 0.0
    for i, key in enumerate(fd):
        for j, (what, mine) in enumerate((("tfront", tf[i]), ("trear", tr[i]))):
            err = np.linalg.norm(fd[key][j][keep] - mine[keep]) / np.linalg.norm(mine[keep])
            print(f"  {what} along {key}: norm-wise relative error {err:.3e}")
            worst = max(worst, err)
            assert err < 1e-5, (key, what, err)
    print(f"H={H} {variant}: worst {worst:.3e}")


def test_nonfinite_inputs_zero_their_block_and_flag():
    H = 10
    v, dy, dphi, seq, st, _, _ = _forward(H, "default")
    d = ct.directions(N, K, 77)
    ok = np.flatnonzero(st >= 0)
    with MpcSolver(horizon=H, device=None) as s:
        clean, flags = _call(s, v, dy, dphi, seq, d, True, status=st)
        assert flags == 0
        for what in ("v", "target", "sequence", "tangent", "tparams"):
            k = int(ok[{"v": 3, "target": 100, "sequence": 200, "tangent": 300, "tparams": 0}[what]])
            a = dict(v=v.copy(), dy=dy.copy(), seq=seq.copy())
            dd = {key: x.copy() for key, x in d.items()}
            if what == "v":
                a["v"][k] = np.nan
            elif what == "target":
                a["dy"][k] = np.inf
            elif what == "sequence":
                a["seq"][2 * H - 1, k] = np.nan
            elif what == "tangent":
                dd["delta_phi"][1, k] = np.nan          # direction 1 of instance k only
            else:
                dd["params"][2, 7] = np.inf             # direction 2 of every instance
            got, flags = _call(s, a["v"], a["dy"], dphi, a["seq"], dd, True, status=st)
            assert flags == capi.FLAG_NONFINITE, what
            gone = np.zeros((K, N), dtype=bool)
            if what == "tangent":
                gone[1, k] = True
            elif what == "tparams":
                gone[2] = True
            else:
                gone[:, k] = True
            for x, c in zip(got, clean):
                x, c = np.moveaxis(x.reshape(K, -1, N), 1, 2), np.moveaxis(c.reshape(K, -1, N), 1, 2)   # [K, N, rows]
                assert not bits(x[gone]).any(), what
                assert np.array_equal(bits(x[~gone]), bits(c[~gone])), what


def test_a_negative_weight_column_is_a_bad_model():
    H = 7
    v, dy, dphi, rows, seq, st = _forward_rows(H, "all")
    d = ct.directions(N, K, 78, rows=True)
    k = int(np.flatnonzero(st >= 0)[5])
    bad = rows.copy()
    bad[0, k] = -1.0
    with MpcSolver(horizon=H, device=None) as s:
        clean, flags = _call(s, v, dy, dphi, seq, d, True, status=st, params_rows=rows)
        assert flags == 0
        got, flags = _call(s, v, dy, dphi, seq, d, True, status=st, params_rows=bad)
        assert flags == capi.FLAG_BAD_MODEL
        wl = bad.copy()
        wl[5, k] = np.nan                                        # the rows entry: a non-finite wheelbase
        _, flags = _call(s, v, dy, dphi, seq, d, False, status=st, params_rows=wl)
        assert flags == capi.FLAG_BAD_MODEL | capi.FLAG_NONFINITE
    rest = np.setdiff1d(np.arange(N), [k])
    for x, c in zip(got, clean):
        assert not bits(x[..., k]).any() and np.abs(c[..., k]).max() > 0
        assert np.array_equal(bits(x[..., rest]), bits(c[..., rest]))


def _raw(h, n=3, H=4, K=2, t=True, mem=capi.HOST, dtype=capi.F64, null=(), rows=False, tparams=False,
         tparams_rows=False, outs=("tfront", "trear", "tsequence"), **over):
    p = capi.default_params(H if 1 <= H <= 64 else 20, dtype=dtype, **over)
    p.horizon = H
    m = max(n, 1) if n < 1024 else 4       # (a refused n is never read: small arrays stand behind it)
    Hh = max(min(H, 64), 1)
    v, dy, dphi = compact_inputs(4, m)
    seq = np.zeros((2 * Hh, m))
    pr = cr.shared_rows(capi.default_params(4), m)
    KK = max(K, 1)
    tv, tp, tpr = np.ones((KK, m)), np.ones((KK, 10)), np.ones((KK, 10, m))
    out = {"tfront": np.full((KK, m), 7.0), "trear": np.full((KK, m), 7.0), "tsequence": np.full((KK, 2 * Hh, m), 7.0)}
    ptr = lambda a, name: None if name in null else a.ctypes.data
    tt = capi.CompactTangents(directions=K, reserved=0, tv=tv.ctypes.data, tparams=tp.ctypes.data if tparams else None,
                              tparams_rows=tpr.ctypes.data if tparams_rows else None)
    flags = C.c_uint32(99)
    rc = capi.load_library().tpc_mpc_solve_batch_compact_exact_forward(
        h, C.byref(p), n, ptr(v, "v"), ptr(dy, "dy"), ptr(dphi, "dphi"), pr.ctypes.data if rows else None,
        ptr(seq, "sequence"), None, C.byref(tt) if t else None,
        *[out[k].ctypes.data if k in outs else None for k in ("tfront", "trear", "tsequence")], C.byref(flags), mem, None)
    return rc, flags.value, out


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


def test_degenerate_calls_and_argument_errors(host_handle):
    h = host_handle
    for kw in ({}, dict(tparams=True), dict(rows=True), dict(rows=True, tparams_rows=True)):
        rc, flags, out = _raw(h, **kw)
        assert (rc, flags) == (0, 0) and all(np.all(a != 7.0) for a in out.values()), kw
    rc, flags, out = _raw(h, n=0)                       # n == 0: OK, flags 0, nothing touched
    assert (rc, flags) == (0, 0) and all(np.all(a == 7.0) for a in out.values())
    rc, flags, out = _raw(h, outs=("trear",))
    assert (rc, flags) == (0, 0) and np.all(out["trear"] != 7.0) and np.all(out["tfront"] == 7.0)
    BAD_ARG, BAD_WEIGHTS, BAD_BOUNDS, BAD_HORIZON, BAD_EPS, NO_DEVICE = 1, 2, 3, 4, 5, 6
    for kw in (dict(t=False), dict(null=("sequence",)), dict(null=("v",)), dict(null=("dy",)), dict(null=("dphi",)),
               dict(K=0), dict(K=-1), dict(n=2 ** 30, K=2), dict(outs=()), dict(dtype=capi.F32), dict(n=-1), dict(mem=5),
               dict(tparams_rows=True), dict(rows=True, tparams=True), dict(step_size=np.inf), dict(wheelbase=0.0)):
        assert _raw(h, **kw)[0] == BAD_ARG, kw
    assert _raw(h, dtype=capi.F32)[0] == BAD_ARG and b"fp64" in capi.load_library().tpc_mpc_last_error(h)
    # without params_rows p is validated as the shared backward validates it; with them its model fields are not read
    assert _raw(h, weight_phi=-1.0)[0] == BAD_WEIGHTS and _raw(h, weight_steering_rear=0.0)[0] == BAD_WEIGHTS
    assert _raw(h, lower=(0.1, -0.1), upper=(0.0, 0.1))[0] == BAD_BOUNDS
    assert _raw(h, rows=True, weight_phi=-1.0, wheelbase=0.0)[:2] == (0, 0)
    assert _raw(h, H=65)[0] == BAD_HORIZON and _raw(h, H=0)[0] == BAD_HORIZON
    assert _raw(h, eps=0.0)[0] == BAD_EPS
    assert _raw(h, mem=capi.DEVICE)[0] == NO_DEVICE
    assert _raw(h, mem=capi.DEVICE, t=False)[0] == BAD_ARG        # reported after the argument checks


def test_the_solver_rejects_what_the_table_forbids():
    n, H = 8, 4
    v, dy, dphi = compact_inputs(H, n)
    seq, rows = np.zeros((2 * H, n)), cr.shared_rows(capi.default_params(H), n)
    with MpcSolver(horizon=H, device=None) as s:
        call = lambda d, **kw: s.solve_batch_compact_exact_forward(v, dy, dphi, seq, d, **kw)
        tf, tr = call({"v": np.ones(n)})
        assert tf.shape == (1, n) and tr.shape == (1, n)
        assert call({"params": np.ones(10)}, want_sequence=True)[2].shape == (1, 2 * H, n)
        assert call({"params_rows": np.ones((10, n))}, params_rows=rows)[0].shape == (1, n)
        assert call({"params_rows": np.ones((2, 10, n)), "v": np.ones((2, n))}, params_rows=rows)[0].shape == (2, n)
        for d, kw in (({"nope": np.ones(n)}, {}), ({"params": np.ones(10)}, dict(params_rows=rows)),
                      ({"params_rows": np.ones((10, n))}, {}), ({"v": np.ones((2, n)), "delta_y": np.ones((3, n))}, {}),
                      ({"v": np.ones((2, n)), "params": np.ones(10)}, {}), ({}, {}),
                      ({"v": np.ones((2, n + 1))}, {}), ({"params": np.ones((1, 9))}, {})):
            with pytest.raises(ValueError):
                call(d, **kw)


def test_symbol_is_declared_and_documented():
    lib = capi.load_library()
    name = "tpc_mpc_solve_batch_compact_exact_forward"
    assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.tpc_mpc_abi_version() == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tpc_mpc.h")) as f:
        text = f.read()
    assert f"int {name}(" in text and "typedef struct tpc_mpc_compact_tangents {" in text
    assert "#define TPC_MPC_ABI_VERSION 5 " in text
    assert "ttvl = (tTv - tvl * tl) / l" in text
    assert [f[0] for f in capi.CompactTangents._fields_] == ["directions", "reserved", "tv", "tdelta_y", "tdelta_phi",
                                                            "tparams", "tparams_rows"]
