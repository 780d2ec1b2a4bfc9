"""GPU tests of the exact compact solve with per-instance parameters (tpc_mpc_solve_batch_compact_exact_rows and its
backward pass, MpcSolver.solve_batch_compact_exact[_backward](params_rows=...), mpc_compact_exact with [.., n]
parameters): the device against the host-only handle bit for bit through the register kernels (H = 4, 5) and the
workspace kernels, forward and backward, HOST and DEVICE memory; the fallback against solve_batch_general +
polish_batch_general on exactly the gathered instances expanded per instance; the device's batch sum, held to the order
mpc_compact_grad.hip documents (cg.device_sum) at the sizes where that order changes shape; the handle's other
entries untouched by a rows call; the autograd function against the raw entries and against the general-form route
mpc_compact(w [4, n], ..., polish=True); one full-size run."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import compact_grad_common as cg
from tests.model import compact_rows_common as cr
from tests.model.compact_exact_common import NAMES, ROUNDS, TOL, bits
from tests.test_compact_grad_gpu import SEAMS, check_params_at_a_seam
from trajectory_controller_amd import MpcSolver, capi, mpc_compact, mpc_compact_exact
from trajectory_controller_amd.synth import compact_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("v", "delta_y", "delta_phi", "params", "params_rows", "kkt_residual")
NS = (1, 63, 65, 300, 4096)   # a lone lane, a partial wavefront, one lane into the second, a partial block, many blocks
SPOILED = (2, 9, 17, 25, 33, 41, 50)          # where the seven cases of cr.INVALID sit from 63 instances on
FWD = ("front", "rear", "sequence", "status", "fell_back", "residual_in", "residual_out")


def _up(a, device=True):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if device else np.ascontiguousarray(a)


def _np(a):
    return None if a is None else np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)


def _inputs(H, n, recipe="all", bad=True):
    v, dy, dphi = (a.copy() for a in compact_inputs(H, n))
    rows = cr.recipe_rows(recipe, H, n)
    invalid = np.zeros(n, dtype=bool)
    if bad and n >= 63:
        rows, v = cr.spoil(rows, v, SPOILED)
        invalid[list(SPOILED[:6])] = True
    return v, dy, dphi, rows, invalid


def _forward(s, v, dy, dphi, rows, device, fallback="none", rounds=ROUNDS):
    out = s.solve_batch_compact_exact(_up(v, device), _up(dy, device), _up(dphi, device), tol=TOL, max_rounds=rounds,
                                      fallback=fallback, want_sequence=True, want_residuals=True,
                                      params_rows=_up(rows, device))
    if device:
        torch.cuda.synchronize()
    return [_np(a) for a in out], s.last_flags


def _backward(s, c, device, want=ALL):
    args = [_up(c[k], device) for k in ("v", "dy", "dphi", "seq", "gf", "gr", "gs")]
    got = s.solve_batch_compact_exact_backward(*args, status=_up(c["st"], device), want=want,
                                               params_rows=_up(c["rows"], device))
    if device:
        torch.cuda.synchronize()
    return {k: _np(a) for k, a in got.items()}, s.last_flags


@functools.lru_cache(maxsize=None)
def _case(H, n, recipe="all"):
    """inputs and the host-only handle's forward and backward, shared by the tests (never modified).  From 63
    instances on: the seven cases of cr.INVALID, and one verified instance whose status is set to -1 for the backward."""
    v, dy, dphi, rows, invalid = _inputs(H, n, recipe)
    gf, gr, gs = cg.grad_in(H, n, 17 + H, sequence=True)
    with MpcSolver(horizon=H, device=None) as s:
        fwd, fflags = _forward(s, v, dy, dphi, rows, False)
        st = fwd[3].copy()
        if n >= 63:
            st[np.flatnonzero(st >= 0)[7]] = -1
        c = dict(v=v, dy=dy, dphi=dphi, rows=rows, seq=fwd[2], st=st, gf=gf, gr=gr, gs=gs, invalid=invalid,
                 fwd=fwd, fflags=fflags)
        c["want"], c["bflags"] = _backward(s, c, False)
    return c


def _same_forward(got, want, cols=None, skip=()):
    for name, a, b in zip(FWD, got, want):
        if name in skip or a is None or b is None:
            continue
        if cols is not None:
            a, b = np.ascontiguousarray(a[..., cols]), np.ascontiguousarray(b[..., cols])
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert a.tobytes() == b.tobytes(), name


# ---- 1. device against host: H = 4, 5 the register kernels, the others the workspace kernels

def _device_equals_host(H, recipe, device, ns):
    bad_flags = capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL
    with MpcSolver(horizon=H, device=0) as s:
        for n in ns:
            c = _case(H, n, recipe)
            got, flags = _forward(s, c["v"], c["dy"], c["dphi"], c["rows"], device)
            _same_forward(got, c["fwd"])
            assert flags == c["fflags"], n
            assert (flags & bad_flags) == (bad_flags if n >= 63 else 0), n
            assert np.all(got[3][c["invalid"]] == -1) and not bits(got[2][:, c["invalid"]]).any()
            if n >= 63:
                assert not c["invalid"][SPOILED[6]]                      # the infinite bound is legal ...
                assert got[3][SPOILED[6]] >= 0 or flags & capi.FLAG_NOT_POLISHED
            back, bflags = _backward(s, c, device)
            for k in cg.PER_INSTANCE:
                assert back[k].tobytes() == c["want"][k].tobytes(), (n, k)
            assert bflags == c["bflags"] == (bad_flags if n >= 63 else 0), n
            excluded = c["st"] < 0
            assert excluded[c["invalid"]].all()
            for k in cg.PER_INSTANCE:
                assert not bits(back[k][..., excluded]).any(), (n, k)
            assert np.all(np.abs(back["params"] - c["want"]["params"]) <= 2 * cg.fsum_bound(back["params_rows"])), n


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H", [1, 4, 5, 7, 10, 20, 40, 64])
def test_device_equals_host_only_handle_bits(H, device):
    _device_equals_host(H, "all", device, NS)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H", [4, 20])
def test_device_equals_host_only_handle_bits_weights_recipe(H, device):
    _device_equals_host(H, "weights", device, (65, 300))


# ---- 2. the fallback

def _reference(s, H, v, dy, dphi, rows, idx, rounds):
    """solve_batch_general (cold, zeroed controls) + polish_batch_general on exactly the instances idx, expanded per
    instance: the entry's outputs in FWD's order and the two calls' flags"""
    th = cr.expand(np.ascontiguousarray(rows[:, idx]), H, v[idx], dy[idx], dphi[idx])
    ins = [_up(th[k]) for k in NAMES]
    u = _up(np.zeros((2 * H, idx.size)))
    u0 = s.solve_batch_general(*ins, controls=u, inputs=2)
    f1 = s.last_flags
    _, st, rin, rout = s.polish_batch_general(*ins, u, tol=TOL, max_rounds=rounds, inputs=2)
    f2 = s.last_flags
    torch.cuda.synchronize()
    u, u0 = _np(u), _np(u0)
    assert np.array_equal(bits(u0[:, _np(st) < 0]), bits(u[:2, _np(st) < 0]))
    return [u[0], u[1], u, _np(st), None, _np(rin), _np(rout)], f1 | f2


def _check_fallback(H, n, recipe, rounds, bad=True):
    v, dy, dphi, rows, invalid = _inputs(H, n, recipe, bad)
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        none, nflags = _forward(s, v, dy, dphi, rows, True, "none", rounds)
        got, flags = _forward(s, v, dy, dphi, rows, True, "solve", rounds)
        fell = got[4]
        assert set(np.unique(fell)) <= {0, 1}
        assert np.array_equal(fell == 1, (none[3] == -1) & ~invalid)
        idx = np.flatnonzero(fell == 1)
        print(f"H={H} n={n} {recipe} rounds={rounds}: fell back {idx.size}, left at -1 by its polish "
              f"{int((got[3][idx] < 0).sum())}, flags {flags:#x}")
        _same_forward(got, none, cols=np.flatnonzero(fell == 0), skip=("fell_back",))
        expect = nflags & ~capi.FLAG_NOT_POLISHED
        if idx.size:
            want, wflags = _reference(s, H, v, dy, dphi, rows, idx, rounds)
            _same_forward([a if a is None else a[..., idx] for a in got], want)
            expect |= wflags
        assert flags == expect
    return got, invalid


@pytest.mark.parametrize("H,recipe", [(5, "all"), (10, "all"), (20, "weights")])
def test_fallback_is_solve_and_polish_on_the_gathered_instances(H, recipe):
    got, invalid = _check_fallback(H, 4096, recipe, ROUNDS)
    assert got[4].sum() > 0
    assert np.all(got[3][invalid] == -1) and not got[4][invalid].any()


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
@pytest.mark.parametrize("H", [4, 10])
def test_everybody_falls_back_without_rounds(H, n):
    got, invalid = _check_fallback(H, n, "all", 0, bad=False)
    assert not invalid.any() and np.array_equal(got[4], np.ones(n, dtype=np.int32))


# ---- 3. dparams on the device

@pytest.mark.parametrize("H", [4, 20])
def test_dparams_is_deterministic_and_within_the_bound_of_any_order(H):
    with MpcSolver(horizon=H, device=0) as s:
        for n in NS:
            c = _case(H, n)
            got, _ = _backward(s, c, True)
            out = got["params_rows"]
            diff = np.abs(got["params"] - cg.fsum_rows(out))
            print(f"H={H} n={n}: max |dparams - fsum| / bound "
                  f"{np.max(diff / np.maximum(cg.fsum_bound(out), 1e-300)):.3f}")
            assert np.all(diff <= cg.fsum_bound(out)), (n, diff, cg.fsum_bound(out))
            again, _ = _backward(s, c, True)
            assert again["params"].tobytes() == got["params"].tobytes(), n
            staged, _ = _backward(s, c, False, want=("params",))     # HOST arrays: the same launches
            assert staged["params"].tobytes() == got["params"].tobytes(), n
            assert got["params"].tobytes() == cg.device_sum(out).tobytes(), n      # the documented order, to the bit


@pytest.mark.parametrize("n", list(SEAMS))
@pytest.mark.parametrize("H", [4, 7], ids=["reg", "ws"])
def test_dparams_is_the_documented_order_where_it_changes_shape(H, n):
    """tests/test_compact_grad_gpu.py's test of the same name through the rows kernels: SEAMS says what each size is;
    the seven cases of cr.INVALID and one more excluded instance put zero rows inside a wavefront (_case)."""
    c = _case(H, n)
    with MpcSolver(horizon=H, device=0) as s:
        flags = check_params_at_a_seam(s, c, _backward, n)
    assert flags == c["bflags"] == capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL


# ---- 4. the handle's other entries: the working sets are shared

def test_other_entries_return_the_same_bytes_around_a_rows_call():
    H, n = 10, 300
    c = _case(H, n)
    v, dy, dphi = compact_inputs(H, n)
    tv, ty, tp = _up(v), _up(dy), _up(dphi)
    th = cr.expand(cr.recipe_rows("all", H, n), H, v, dy, dphi)
    ins = [_up(th[k]) for k in NAMES]
    g = _up(cg.expanded_gradient(H, n, c["gf"], c["gr"], c["gs"]))

    def others(s):
        out = list(s.solve_batch_compact_exact(tv, ty, tp, tol=TOL, max_rounds=ROUNDS, want_sequence=True,
                                               want_residuals=True))
        out += list(s.solve_batch_compact_exact_backward(tv, ty, tp, out[2], _up(c["gf"]), _up(c["gr"]), _up(c["gs"]),
                                                         status=out[3], want=ALL).values())
        u = torch.zeros((2 * H, n), dtype=torch.float64, device=DEV)
        out += list(s.solve_batch_general_backward(*ins, u, g, inputs=2).values())
        torch.cuda.synchronize()
        return [_np(a).tobytes() for a in out if a is not None]

    with MpcSolver(horizon=H, device=0) as s:
        before = others(s)
        got, _ = _forward(s, c["v"], c["dy"], c["dphi"], c["rows"], True, "solve")
        back, _ = _backward(s, c, True)
        assert others(s) == before
        again, _ = _forward(s, c["v"], c["dy"], c["dphi"], c["rows"], True, "solve")
        _same_forward(again, got)
        again, _ = _backward(s, c, True)
        for k in ALL:
            assert again[k].tobytes() == back[k].tobytes(), k


# ---- 5. autograd

@pytest.mark.parametrize("mixed", [False, True], ids=["weights", "mixed"])
@pytest.mark.parametrize("H", [4, 20])
def test_autograd_equals_the_raw_entries(H, mixed):
    n = 300
    v, dy, dphi = compact_inputs(H, n)
    rows = cr.recipe_rows("all" if mixed else "weights", H, n)
    rng = np.random.default_rng(4)
    cf, cb = _up(rng.standard_normal(n)), _up(rng.standard_normal(n))
    with MpcSolver(horizon=H, device=0) as s:
        p = s.params
        if mixed:      # T and l stay shared: the solver's own l, a given T that requires grad
            rows[cr.T], rows[cr.L] = 0.07, p.wheelbase
        tv, ty, tp = (_up(a).requires_grad_() for a in (v, dy, dphi))
        weights = _up(rows[cr.W]).requires_grad_()
        kw = {}
        if mixed:
            kw = dict(lower=_up(rows[cr.LO]).requires_grad_(), upper=_up(rows[cr.HI]),
                      step_size=torch.tensor(0.07, dtype=torch.float64, requires_grad=True))      # on the CPU
        front, rear = mpc_compact_exact(s, tv, ty, tp, weights=weights, tol=TOL, max_rounds=ROUNDS, **kw)
        trows = _up(rows)
        rf, rr, seq, st, _ = s.solve_batch_compact_exact(tv.detach(), ty.detach(), tp.detach(), tol=TOL,
                                                         max_rounds=ROUNDS, want_sequence=True, params_rows=trows)
        torch.cuda.synchronize()
        assert _np(front.detach()).tobytes() == _np(rf).tobytes() and _np(rear.detach()).tobytes() == _np(rr).tobytes()
        (cf * front + cb * rear).sum().backward()
        raw = s.solve_batch_compact_exact_backward(tv.detach(), ty.detach(), tp.detach(), seq, cf, cb, status=st,
                                                   want=ALL, params_rows=trows)
        torch.cuda.synchronize()
        for t, k in ((tv, "v"), (ty, "delta_y"), (tp, "delta_phi")):
            assert _np(t.grad).tobytes() == _np(raw[k]).tobytes(), k
        assert tuple(weights.grad.shape) == (4, n)
        assert _np(weights.grad).tobytes() == _np(raw["params_rows"][cr.W]).tobytes()
        if mixed:
            assert _np(kw["lower"].grad).tobytes() == _np(raw["params_rows"][cr.LO]).tobytes()
            assert kw["upper"].grad is None
            step = kw["step_size"]
            assert step.grad.device.type == "cpu" and step.grad.shape == ()
            assert _np(step.grad).tobytes() == _np(raw["params"][cr.T]).tobytes()
    # a call with no per-instance parameter takes the shared path: [4] weights are not rows, whatever n is
    with MpcSolver(horizon=H, device=0) as s:
        w4 = torch.tensor([20.0, 7.0, 0.0005, 10.0], dtype=torch.float64)
        front, _ = mpc_compact_exact(s, _up(v[:4]), _up(dy[:4]), _up(dphi[:4]), weights=w4, tol=TOL, max_rounds=ROUNDS)
        want, _, _, _ = s.solve_batch_compact_exact(_up(v[:4]), _up(dy[:4]), _up(dphi[:4]), tol=TOL, max_rounds=ROUNDS)
        assert _np(front).tobytes() == _np(want).tobytes()


@pytest.mark.parametrize("H", [4, 20])
def test_gradients_agree_with_mpc_compact_polished(H):
    """Both routes take the same derivative (qp_step on the expanded model) at sequences that agree to rounding, so the
    bound is section 20's, 1e-8 norm-wise.  The loss is a random linear one restricted to the instances both routes
    verify."""
    n = 4096
    v, dy, dphi = compact_inputs(H, n)
    rows = cr.recipe_rows("weights", H, n)
    rng = np.random.default_rng(8)
    cf, cb = rng.standard_normal(n), rng.standard_normal(n)
    with MpcSolver(horizon=H, device=0) as s:
        p = s.params
        th = cr.expand(rows, H, v, dy, dphi)
        ins = [_up(th[k]) for k in NAMES]
        u = torch.zeros((2 * H, n), dtype=torch.float64, device=DEV)
        s.solve_batch_general(*ins, controls=u, inputs=2)
        _, pst, _, _ = s.polish_batch_general(*ins, u, tol=TOL, max_rounds=8, inputs=2)      # polish=True is (1e-9, 8)
        _, _, est, _ = s.solve_batch_compact_exact(_up(v), _up(dy), _up(dphi), tol=TOL, max_rounds=ROUNDS,
                                                   params_rows=_up(rows))
        both = (pst >= 0) & (est >= 0)
        assert int(both.sum()) >= 0.95 * n
        mf, mr = _up(cf) * both, _up(cb) * both
        grads = {}
        for route in ("exact", "general"):
            tv, ty, tp = (_up(a).requires_grad_() for a in (v, dy, dphi))
            w = _up(rows[cr.W]).requires_grad_()
            if route == "exact":
                front, rear = mpc_compact_exact(s, tv, ty, tp, weights=w, tol=TOL, max_rounds=ROUNDS, fallback="solve")
            else:
                front, rear = mpc_compact(s, tv, ty, tp, w, step_size=p.step_size, wheelbase=p.wheelbase,
                                          lower=tuple(p.lower), upper=tuple(p.upper), polish=True)
            (mf * front + mr * rear).sum().backward()
            torch.cuda.synchronize()
            grads[route] = [_np(t.grad) for t in (tv, ty, tp, w)]
    keep = _np(both)
    worst = 0.0
    for name, a, b in zip(("v", "delta_y", "delta_phi", "weights"), grads["exact"], grads["general"]):
        a, b = a[..., keep], b[..., keep]
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(f"H={H} d{name}: norm-wise relative difference {rel:.3e}")
        worst = max(worst, rel)
    print(f"H={H}: both verify {int(keep.sum())}/{n}, worst {worst:.3e}")
    assert worst <= 1e-8


# ---- 6. full size

def test_full_size_call():
    H, n = 20, 262144
    v, dy, dphi = compact_inputs(H, n)
    rows = cr.recipe_rows("all", H, n)
    gf, gr, gs = cg.grad_in(H, n, 2, sequence=True)
    with MpcSolver(horizon=H, device=0) as s:
        tv, ty, tp, tr = _up(v), _up(dy), _up(dphi), _up(rows)
        _, _, seq, st, fell, rin, rout = s.solve_batch_compact_exact(tv, ty, tp, tol=TOL, max_rounds=ROUNDS,
                                                                    want_sequence=True, want_residuals=True,
                                                                    params_rows=tr)
        fflags = s.last_flags
        got = s.solve_batch_compact_exact_backward(tv, ty, tp, seq, _up(gf), _up(gr), _up(gs), status=st, want=ALL,
                                                   params_rows=tr)
        torch.cuda.synchronize()
        flags = s.last_flags
    st, fell = _np(st), _np(fell)
    print(f"262144 x N=20, recipe all: forward flags {fflags:#x}, backward flags {flags:#x}, fell back "
          f"{int(fell.sum())}, left unverified {int((st < 0).sum())}")
    assert flags == 0 and not fflags & (capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL)
    assert 0 < fell.sum() <= 0.20 * n
    assert bool((st < 0).any()) == bool(fflags & capi.FLAG_NOT_POLISHED)
    assert np.all(_np(rout)[st >= 0] <= TOL)
    lo, hi = np.tile(rows[cr.LO], (H, 1)), np.tile(rows[cr.HI], (H, 1))
    assert np.all((_np(seq) >= lo) & (_np(seq) <= hi))
    for k in ALL:
        assert np.all(np.isfinite(_np(got[k]))), k
    out = _np(got["params_rows"])
    assert np.all(np.abs(_np(got["params"]) - cg.fsum_rows(out)) <= cg.fsum_bound(out))
    assert _np(got["params"]).tobytes() == cg.device_sum(out).tobytes()      # 256-lane blocks, 1024 partials
