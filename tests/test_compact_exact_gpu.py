"""GPU tests of the exact compact solve (tpc_mpc_solve_batch_compact_exact, MpcSolver.solve_batch_compact_exact): the
device against the host-only handle bit for bit through the register kernels (H = 4, 5) and the workspace kernel under
every controller model of VARIANTS, the fallback against solve_batch_general + polish_batch_general on exactly the
gathered instances bit for bit (from the register kernels and under non-default models too), every subset of the
optional outputs through the C entry, the AUTO fallback against the LANE one, the other entries of the handle untouched
by an exact call, and one full-size run."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model.compact_exact_common import N, NAMES, ROUNDS, TOL, VARIANTS, bits, expand
from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd.synth import compact_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("front", "rear", "sequence", "status", "fell_back", "residual_in", "residual_out")


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if device else np.ascontiguousarray(a)


def _np(a):
    return None if a is None else np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)


def _exact(s, v, dy, dphi, device, fallback, rounds=ROUNDS, **over):
    """every output of solve_batch_compact_exact as numpy arrays in FIELDS' order, and the flags"""
    out = s.solve_batch_compact_exact(_up(v, device), _up(dy, device), _up(dphi, device), tol=TOL, max_rounds=rounds,
                                      fallback=fallback, want_sequence=True, want_residuals=True, **over)
    if device:
        torch.cuda.synchronize()
    return [_np(a) for a in out], s.last_flags


def _inputs(H, n, bad=True):
    """the first n instances of the horizon's stream; from 63 instances on, one NaN speed and one infinite target"""
    v, dy, dphi = (a.copy() for a in compact_inputs(H, n))
    invalid = np.zeros(n, dtype=bool)
    if bad and n >= 63:
        v[5], dphi[n - 2] = np.nan, np.inf
        invalid[[5, n - 2]] = True
    return v, dy, dphi, invalid


@functools.lru_cache(maxsize=None)
def _host(H, n, rounds=ROUNDS, variant="default"):
    v, dy, dphi, _ = _inputs(H, n)
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        return _exact(s, v, dy, dphi, False, "none", rounds)


def _same(got, want, cols=None, skip=()):
    for name, a, b in zip(FIELDS, got, want):
        if name in skip or a is None or b is None:
            continue
        if cols is not None:
            a, b = np.ascontiguousarray(a[..., cols]), np.ascontiguousarray(b[..., cols])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), name


# ---- 1. device against host: H = 4, 5 the register kernels, 10 / 20 / 40 and the unspecialised 7 the workspace kernel

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", [1, 63, 65, N])
@pytest.mark.parametrize("H", [4, 5, 7, 10, 20, 40])
def test_device_equals_host_only_handle_bits(H, n, device):
    v, dy, dphi, invalid = _inputs(H, n)
    want, wflags = _host(H, n)
    with MpcSolver(horizon=H, device=0) as s:
        got, flags = _exact(s, v, dy, dphi, device, "none")
    print(f"H={H} n={n}: unverified {int((want[3] < 0).sum()) - int(invalid.sum())}, flags {flags:#x}")
    _same(got, want)
    assert flags == wflags
    assert bool(flags & capi.FLAG_NONFINITE) == bool(invalid.any())


# every model through the register kernels (H = 4, 5) and the workspace kernel (H = 7, 20): unequal bounds, a box that
# excludes U = 0, a pinned input; and the horizons 1, 2 and 64 of the workspace kernel with the default model
PER_MODEL = [(H, n, variant) for variant in VARIANTS for H in (4, 5, 7, 20) for n in (65, N)] + \
    [(H, 65, "default") for H in (1, 2, 64)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H,n,variant", PER_MODEL)
def test_device_equals_host_only_handle_bits_per_model(H, n, variant, device):
    v, dy, dphi, invalid = _inputs(H, n)
    want, wflags = _host(H, n, variant=variant)
    with MpcSolver(horizon=H, device=0, **VARIANTS[variant]) as s:
        got, flags = _exact(s, v, dy, dphi, device, "none")
    print(f"H={H} n={n} {variant}: unverified {int((want[3] < 0).sum()) - int(invalid.sum())}, flags {flags:#x}")
    _same(got, want)
    assert flags == wflags
    assert bool(flags & capi.FLAG_NONFINITE) == bool(invalid.any())


# ---- 2. the fallback

def _reference(s, H, v, dy, dphi, idx, device, rounds, **over):
    """solve_batch_general (cold, zeroed controls) + polish_batch_general on exactly the instances idx, expanded:
    (u0 [2, m], sequence, status, residual_in, residual_out) and the two calls' flags"""
    th = expand(s._params(**over), H, v[idx], dy[idx], dphi[idx])
    ins = [_up(th[k], device) for k in NAMES]
    u = _up(np.zeros((2 * H, idx.size)), device)
    u0 = s.solve_batch_general(*ins, controls=u, inputs=2, **over)
    f1 = s.last_flags
    _, st, rin, rout = s.polish_batch_general(*ins, u, tol=TOL, max_rounds=rounds, inputs=2, **over)
    f2 = s.last_flags
    if device:
        torch.cuda.synchronize()
    u = _np(u)
    u0 = _np(u0)
    # the entry returns the polish's u0: row 0 of the polished sequence, the solver's where the polish failed
    assert np.array_equal(bits(u0[:, _np(st) < 0]), bits(u[:2, _np(st) < 0]))
    return [u[0], u[1], u, _np(st), None, _np(rin), _np(rout)], f1 | f2


def _check_fallback(H, n, device, rounds, algo="lane", variant="default", bad=True):
    v, dy, dphi, invalid = _inputs(H, n, bad)
    with MpcSolver(horizon=H, device=0, algo=algo, **VARIANTS[variant]) as s:
        none, nflags = _exact(s, v, dy, dphi, device, "none", rounds)
        got, flags = _exact(s, v, dy, dphi, device, "solve", rounds)
        fell = got[4]
        assert set(np.unique(fell)) <= {0, 1}
        assert np.array_equal(fell == 1, (none[3] == -1) & ~invalid)
        idx = np.flatnonzero(fell == 1)
        print(f"H={H} n={n} rounds={rounds}: fell back {idx.size}, left at -1 by its polish "
              f"{int((got[3][idx] < 0).sum())}, flags {flags:#x}")
        _same(got, none, cols=np.flatnonzero(fell == 0), skip=("fell_back",))
        expect = nflags & ~capi.FLAG_NOT_POLISHED
        if idx.size:
            want, wflags = _reference(s, H, v, dy, dphi, idx, device, rounds)      # the variant: the handle's params
            _same([a if a is None else a[..., idx] for a in got], want)
            expect |= wflags
        assert flags == expect
    return got, flags, invalid


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H", [10, 20])
def test_fallback_is_solve_and_polish_on_the_gathered_instances(H, device):
    got, flags, invalid = _check_fallback(H, N, device, ROUNDS)
    assert got[4].sum() > 0
    left = (got[3] < 0) & ~invalid
    assert not left[got[4] == 0].any()                                  # verified in phase 1, or sent to the fallback
    assert bool(left.any()) == bool(flags & capi.FLAG_NOT_POLISHED)     # ... and verified there, or flagged


def test_nobody_falls_back_at_the_reference_horizon():
    got, flags, invalid = _check_fallback(4, N, True, ROUNDS)
    assert got[4].sum() == 0 and flags == capi.FLAG_NONFINITE and np.all((got[3] >= 0) | invalid)


def test_everybody_falls_back_without_rounds():
    got, flags, invalid = _check_fallback(10, 1000, True, 0)
    assert np.array_equal(got[4] == 1, ~invalid)


# the host path leaves 58, 35, 167, 1, 631 and 282 of these batches unverified (without the two poisoned instances of
# _inputs, which move a count by at most two): the queue fills from the register kernels, the gather kernel writes
# unequal bounds and other weights, and (5, weights) is a batch of one through gather and scatter (one live lane)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H,variant", [(4, "asymmetric"), (4, "offset"), (5, "asymmetric"), (5, "weights"),
                                       (10, "asymmetric"), (20, "weights")])
def test_fallback_from_the_register_kernels_and_under_other_models(H, variant, device):
    got, flags, invalid = _check_fallback(H, N, device, ROUNDS, variant=variant)
    count = int(got[4].sum())
    assert count > 0
    if (H, variant) != (5, "weights"):
        assert count % 64 != 0          # the last wavefront of the gathered batch is partly live
    left = (got[3] < 0) & ~invalid
    assert not left[got[4] == 0].any()
    assert bool(left.any()) == bool(flags & capi.FLAG_NOT_POLISHED)


# max_rounds = 0 verifies nobody: the whole batch goes through a register kernel's queue, whatever order it comes out in
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H,n,variant", [(H, n, "default") for H in (4, 5) for n in (1, 64, 65, 1000)] +
                         [(4, 65, "asymmetric"), (5, 65, "asymmetric")])
def test_everybody_falls_back_from_a_register_kernel(H, n, variant, device):
    got, flags, invalid = _check_fallback(H, n, device, 0, variant=variant, bad=False)
    # _check_fallback has compared every instance with fell_back = 1 with _reference on exactly those: all of them
    assert not invalid.any() and np.array_equal(got[4], np.ones(n, dtype=np.int32))


# ---- 2b. every subset of the optional outputs, through the C entry

OPTIONAL = ("sequence_out", "residual_in", "residual_out", "status", "fell_back")


def _raw_exact(s, H, v, dy, dphi, device, fallback, present, sentinel=-777.0):
    """tpc_mpc_solve_batch_compact_exact with exactly the optional outputs named in `present`, every given output filled
    with a sentinel before the call: ({name: numpy array}, flags)"""
    n = v.shape[0]
    ins = [_up(a, device) for a in (v, dy, dphi)]
    f64 = lambda *shape: _up(np.full(shape, sentinel), device)
    i32 = lambda: _up(np.full(n, -7, dtype=np.int32), device)
    out = dict(front=f64(n), rear=f64(n))
    out.update({k: make() for k, make in (("sequence_out", lambda: f64(2 * H, n)), ("residual_in", lambda: f64(n)),
                                          ("residual_out", lambda: f64(n)), ("status", i32), ("fell_back", i32))
                if k in present})
    ptr = lambda a: None if a is None else (a.data_ptr() if device else a.ctypes.data)
    q = capi.Polish(tol=TOL, max_rounds=ROUNDS, reserved=0, status=ptr(out.get("status")),
                    residual_in=ptr(out.get("residual_in")), residual_out=ptr(out.get("residual_out")))
    flags = C.c_uint32(99)
    rc = s._lib.tpc_mpc_solve_batch_compact_exact(
        s._h, C.byref(s._params()), n, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), C.byref(q),
        capi.NEWTON_FALLBACKS[fallback], ptr(out["front"]), ptr(out["rear"]), ptr(out.get("sequence_out")),
        ptr(out.get("fell_back")), C.byref(flags), capi.DEVICE if device else capi.HOST, None)
    assert rc == 0
    if device:
        torch.cuda.synchronize()
    return {k: _np(a) for k, a in out.items()}, flags.value


@pytest.mark.parametrize("fallback", ["solve", "none"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H", [5, 7])
def test_every_subset_of_the_optional_outputs(H, device, fallback):
    """The HOST staging packs its rows by which outputs are present and the scatter kernel writes what is present: the
    outputs of each of the 32 subsets equal the all-present call's bits, and no given row is left unwritten."""
    n = 65
    v, dy, dphi, _ = _inputs(H, n)
    with MpcSolver(horizon=H, device=0, algo="lane", **VARIANTS["asymmetric"]) as s:
        full, fflags = _raw_exact(s, H, v, dy, dphi, device, fallback, OPTIONAL)
        assert np.all(full["status"] != -7) and np.all(full["fell_back"] != -7)
        assert not any(np.any(full[k] == -777.0) for k in full if k not in ("status", "fell_back"))
        if fallback == "solve":
            assert full["fell_back"].sum() > 0      # the scatter kernel ran
        else:
            assert not full["fell_back"].any() and (full["status"] < 0).sum() > 2
        for r in range(len(OPTIONAL) + 1):
            for present in itertools.combinations(OPTIONAL, r):
                got, flags = _raw_exact(s, H, v, dy, dphi, device, fallback, present)
                assert flags == fflags, present
                assert set(got) == {"front", "rear"} | set(present)
                for k, a in got.items():
                    assert a.dtype == full[k].dtype and a.tobytes() == full[k].tobytes(), (present, k)


def test_auto_fallback_agrees_with_the_lane_fallback():
    H = 20
    v, dy, dphi, invalid = _inputs(H, N)
    res = {}
    for algo in ("lane", "auto"):
        with MpcSolver(horizon=H, device=0, algo=algo) as s:
            res[algo] = _exact(s, v, dy, dphi, True, "solve")
    (lane, lflags), (auto, aflags) = res["lane"], res["auto"]
    assert np.array_equal(auto[4], lane[4])
    left = (auto[3] < 0) & ~invalid
    print(f"AUTO fallback: {int(auto[4].sum())} fell back, {int(left.sum())} left at -1, flags {aflags:#x}")
    assert bool(left.any()) == bool(aflags & capi.FLAG_NOT_POLISHED)      # verified, or flagged
    assert bool(aflags & capi.FLAG_NONFINITE)
    both = (auto[3] >= 0) & (lane[3] >= 0)
    assert both[auto[4] == 1].any()
    err = max(np.abs(auto[0] - lane[0])[both].max(), np.abs(auto[1] - lane[1])[both].max())
    print(f"max |u0(AUTO fallback) - u0(LANE fallback)| {err:.3e}")
    assert err <= 1e-9


# ---- 3. the handle's other entries: the gradient workspace and the Newton working set are shared

def test_other_entries_return_the_same_bytes_around_an_exact_call():
    from tests.model import mpc_rollout_dense as rd
    from tests.test_rollout_newton_host import soa_inputs
    H, n, S = 10, 300, 4
    v, dy, dphi, _ = _inputs(H, n)
    tv, ty, tp = (_up(a, True) for a in (v, dy, dphi))
    th = expand(capi.default_params(H), H, *compact_inputs(H, n))
    ins = [_up(th[k], True) for k in NAMES]
    rth, nlt = rd.batch(2, H, S, n, seed=11, with_nlt=True)
    rins, rnl = soa_inputs(rth, nlt, n)
    rins, rnl = [_up(a, True) for a in rins], _up(rnl, True)

    def others(s):
        out = list(s.solve_batch_compact(tv, ty, tp, want_iters=True))
        u = torch.zeros((2 * H, n), dtype=torch.float64, device=DEV)
        u0 = s.solve_batch_general(*ins, controls=u, inputs=2)
        out += [u0] + list(s.polish_batch_general(*ins, u, tol=TOL, max_rounds=ROUNDS, inputs=2))
        out += [a for a in s.rollout_newton(S, *rins, rnl, inputs=2, tol=TOL, max_rounds=ROUNDS, fallback="solve",
                                            want_iters=True) if a is not None]
        torch.cuda.synchronize()
        return [_np(a).tobytes() for a in out]

    with MpcSolver(horizon=H, device=0) as s:
        before = others(s)
        for fallback in ("solve", "none"):
            got, _ = _exact(s, v, dy, dphi, True, fallback)
            assert others(s) == before, fallback
        again, _ = _exact(s, v, dy, dphi, True, "none")
        _same(again, got)


# ---- 4. full size

def test_full_size_call():
    H, n = 20, 262144
    v, dy, dphi = compact_inputs(H, n)
    with MpcSolver(horizon=H, device=0) as s:
        front, rear, st, fell = s.solve_batch_compact_exact(_up(v, True), _up(dy, True), _up(dphi, True), tol=TOL,
                                                            max_rounds=ROUNDS)
        torch.cuda.synchronize()
        flags = s.last_flags
    st, fell = _np(st), _np(fell)
    share = float(fell.mean())
    print(f"262144 x N=20: fell back {int(fell.sum())} ({100 * share:.2f} %), left at -1 {int((st < 0).sum())}, "
          f"flags {flags:#x}, rounds histogram {np.bincount(st[st >= 0], minlength=ROUNDS + 1).tolist()}")
    assert np.all(st >= 0) or bool(flags & capi.FLAG_NOT_POLISHED)
    assert flags & ~(capi.FLAG_NOT_POLISHED | capi.FLAG_MAX_ITER) == 0
    assert share <= 0.10
    assert np.all(np.isfinite(_np(front))) and np.all(np.isfinite(_np(rear)))
