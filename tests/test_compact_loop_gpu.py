"""GPU tests of the compact closed loop (tpc_mpc_rollout_compact_exact, MpcSolver.rollout_compact_exact,
mpc_rollout_compact): the device against the host-only handle byte for byte through the register kernels (H = 4, 5) and
the workspace kernel, in HOST and DEVICE memory and at the block thresholds; the fallback against rollout_polished on
exactly the gathered instances, expanded, bit for bit; the AUTO fallback against the LANE one; the handle's other
entries untouched by a loop call, and a call on a side stream; the autograd function against mpc_rollout on the
expanded tensors and against central differences; one large call."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import compact_loop_common as cl
from tests.model.compact_loop_common import NAMES, ROUNDS, ROWS, TOL, VARIANTS, bits
from trajectory_controller_amd import MpcSolver, capi, mpc_rollout, mpc_rollout_compact
from trajectory_controller_amd.synth import compact_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a, device):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if device else np.ascontiguousarray(a)


def _np(a):
    return None if a is None else np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)


def _loop(s, S, v, dy, dphi, x0, device, fallback="none", rounds=ROUNDS, tol=TOL, **over):
    """every row of rollout_compact_exact as numpy arrays, and the flags"""
    n = v.shape[0]
    rin, rout = _up(np.full((S, n), 7.0), device), _up(np.full((S, n), 7.0), device)
    out = s.rollout_compact_exact(S, _up(v, device), _up(dy, device), _up(dphi, device), _up(x0, device), tol=tol,
                                  max_rounds=rounds, fallback=fallback, residuals=(rin, rout), **over)
    if device:
        torch.cuda.synchronize()
    c = dict(zip(("controls", "states", "sequences", "status", "first"), (_np(a) for a in out)))
    c.update(rin=_np(rin), rout=_np(rout), flags=s.last_flags)
    return c


def _inputs(H, n, with_x0, bad=True):
    """the first n instances of the horizon's stream; from 63 instances on, one NaN speed"""
    v, dy, dphi = (a.copy() for a in compact_inputs(H, n))
    invalid = np.zeros(n, dtype=bool)
    if bad and n >= 63:
        v[5] = np.nan
        invalid[5] = True
    return v, dy, dphi, (cl.start_states(H, n) if with_x0 else None), invalid


@functools.lru_cache(maxsize=None)
def _host(H, n, S, variant="default", with_x0=False, rounds=ROUNDS, bad=True):
    v, dy, dphi, x0, _ = _inputs(H, n, with_x0, bad)
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        return _loop(s, S, v, dy, dphi, x0, False, rounds=rounds)


# ---- 1. device against host: H = 4, 5 the register kernels, 1 / 7 / 20 / 64 the workspace kernel

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("with_x0", [False, True], ids=["x0=null", "x0"])
@pytest.mark.parametrize("variant", ["default", "weights", "offset"])
@pytest.mark.parametrize("H", [4, 5, 1, 7, 20, 64])
def test_device_equals_host_only_handle_bytes(H, variant, with_x0, device):
    with MpcSolver(horizon=H, device=0, **VARIANTS[variant]) as s:
        for n in (1, 63, 65, 300):
            for S in (1, 5):
                v, dy, dphi, x0, invalid = _inputs(H, n, with_x0)
                want = _host(H, n, S, variant, with_x0)
                got = _loop(s, S, v, dy, dphi, x0, device)
                assert cl.same_rows(got, want) == [], (n, S)
                assert got["flags"] == want["flags"], (n, S)
                assert bool(got["flags"] & capi.FLAG_NONFINITE) == bool(invalid.any())
                assert np.all(got["first"][invalid] == 0)


# the launcher's block is the largest of 256, 128, 64 that gives every CU a block: 32 641 lanes are the last batch on
# blocks of 64, 65 280 the last on 128 and 65 281 the first on 256
@pytest.mark.parametrize("H,n", [(4, 32641), (4, 65280), (4, 65281), (7, 65281)])
def test_block_thresholds(H, n):
    S = 2
    v, dy, dphi, x0, _ = _inputs(H, n, True)
    want = _host(H, n, S, "default", True)
    with MpcSolver(horizon=H, device=0) as s:
        got = _loop(s, S, v, dy, dphi, x0, True)
    assert cl.same_rows(got, want) == [] and got["flags"] == want["flags"]


# ---- 2. the fallback

def _check_fallback(H, S, n, variant, device, rounds=ROUNDS, algo="lane", with_x0=True, bad=True):
    v, dy, dphi, x0, invalid = _inputs(H, n, with_x0, bad)
    with MpcSolver(horizon=H, device=0, algo=algo, **VARIANTS[variant]) as s:
        none = _loop(s, S, v, dy, dphi, x0, device, "none", rounds)
        got = _loop(s, S, v, dy, dphi, x0, device, "solve", rounds)
        assert np.array_equal(got["first"], none["first"])                # first_unverified keeps phase 1's value
        fell = (none["first"] < S) & ~invalid
        idx = np.flatnonzero(fell)
        assert cl.same_rows(got, none, cols=np.flatnonzero(~fell)) == []  # everyone else keeps their FALLBACK_NONE bits
        expect = none["flags"] & ~capi.FLAG_NOT_POLISHED
        left = 0
        if idx.size:
            want = cl.reference(s, S, v[idx], dy[idx], dphi[idx], None if x0 is None else x0[:, idx], rounds=rounds,
                                polished=True)
            assert cl.same_rows({k: got[k][..., idx] for k in ROWS[:-1]}, want, rows=ROWS[:-1]) == []
            expect |= want["flags"]
            left = int((want["status"] < 0).sum())
        print(f"H={H} S={S} n={n} {variant} rounds={rounds}: fell back {idx.size}, (instance, step) pairs its loop left "
              f"at -1 {left}, flags {got['flags']:#x}")
        assert got["flags"] == expect                                     # the OR of the parts
    return got, fell, invalid


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("H,S,n,variant", [(10, 10, 4096, "weights"), (20, 4, 4096, "default"),
                                           (4, 8, 1000, "asymmetric")])
def test_fallback_is_rollout_polished_on_the_gathered_instances(H, S, n, variant, device):
    got, fell, invalid = _check_fallback(H, S, n, variant, device)
    assert fell.sum() > 0 and invalid.sum() == 1
    assert bool(got["flags"] & capi.FLAG_NONFINITE) and np.all(got["status"][:, invalid] == -1)


def test_nobody_falls_back_at_the_reference_horizon():
    got, fell, _ = _check_fallback(4, 8, 4096, "default", True, with_x0=False, bad=False)
    assert fell.sum() == 0 and got["flags"] == 0 and np.all(got["status"] >= 0)


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("H", [4, 7])
def test_everybody_falls_back_without_rounds(H, n):
    got, fell, _ = _check_fallback(H, 3, n, "default", True, rounds=0, bad=False)
    assert fell.all() and np.all(got["first"] == 0)


# ... and from HOST arrays: the staged slots go through gather, the polished loop and scatter with every instance queued
@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("H", [4, 7])
def test_everybody_falls_back_without_rounds_from_host_arrays(H, n):
    got, fell, _ = _check_fallback(H, 3, n, "default", False, rounds=0, bad=False)
    assert fell.all() and np.all(got["first"] == 0)


def test_auto_fallback_agrees_with_the_lane_fallback():
    H, S, n = 10, 10, 4096
    v, dy, dphi, x0, invalid = _inputs(H, n, True)
    res = {}
    for algo in ("lane", "auto"):
        with MpcSolver(horizon=H, device=0, algo=algo, **VARIANTS["weights"]) as s:
            res[algo] = _loop(s, S, v, dy, dphi, x0, True, "solve")
    lane, auto = res["lane"], res["auto"]
    assert np.array_equal(auto["first"], lane["first"])
    both = (auto["status"] >= 0) & (lane["status"] >= 0)                  # (step, instance) pairs both loops verified
    fell = (lane["first"] < S) & ~invalid
    assert fell.sum() > 0 and both[:, fell].any()
    rows = np.repeat(both, 2, axis=0)
    err = max(float(np.abs(auto[k] - lane[k])[rows].max()) for k in ("controls", "states"))
    print(f"{int(fell.sum())} fell back; max |AUTO fallback - LANE fallback| over controls and states {err:.3e}")
    assert err <= 1e-9


# ---- 3. the handle's other entries: the gradient workspace and the Newton working set are shared

def test_other_entries_return_the_same_bytes_around_a_loop_call():
    from tests.model import mpc_rollout_dense as rd
    from tests.test_rollout_newton_host import soa_inputs
    H, n, S = 10, 300, 4
    v, dy, dphi, x0, _ = _inputs(H, n, True)
    tv, ty, tp = (_up(a, True) for a in (v, dy, dphi))
    rth, nlt = rd.batch(2, H, S, n, seed=11, with_nlt=True)
    rins, rnl = soa_inputs(rth, nlt, n)
    rins, rnl = [_up(a, True) for a in rins], _up(rnl, True)

    def others(s):
        out = list(s.solve_batch_compact(tv, ty, tp, want_iters=True))
        out += [a for a in s.solve_batch_compact_exact(tv, ty, tp, tol=TOL, max_rounds=ROUNDS, want_sequence=True)]
        out += [a for a in s.rollout_newton(S, *rins, rnl, inputs=2, tol=TOL, max_rounds=ROUNDS, fallback="solve",
                                            want_iters=True) if a is not None]
        torch.cuda.synchronize()
        return [_np(a).tobytes() for a in out]

    with MpcSolver(horizon=H, device=0, **VARIANTS["weights"]) as s:
        before = others(s)
        got = {}
        for fallback in ("solve", "none"):
            got[fallback] = _loop(s, S, v, dy, dphi, x0, True, fallback)
            assert others(s) == before, fallback
        assert cl.same_rows(_loop(s, S, v, dy, dphi, x0, True, "none"), got["none"]) == []
        # a side stream, no flags: asynchronous, the same controls / states / sequences
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c, x, q, st, first = s.rollout_compact_exact(S, tv, ty, tp, _up(x0, True), tol=TOL, max_rounds=ROUNDS,
                                                         fallback="none", want_status=False)
        side.synchronize()
        assert st is None and first is None and s.last_flags == 0
        for name, a in (("controls", c), ("states", x), ("sequences", q)):
            assert np.array_equal(bits(_np(a)), bits(got["none"][name])), name
        assert others(s) == before


# ---- 4. autograd

def _leaves(H, n, variant, with_x0=True):
    v, dy, dphi, x0, _ = _inputs(H, n, with_x0, bad=False)
    p = capi.default_params(H, **VARIANTS[variant])
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV, requires_grad=True)
    return dict(v=t(v), delta_y=t(dy), delta_phi=t(dphi), x0=t(x0),
                weights=t([p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear]),
                step_size=t(p.step_size), wheelbase=t(p.wheelbase), lower=t(list(p.lower)), upper=t(list(p.upper)))


def _expanded_tensors(L, H):
    """mpc_compact's expansion (autograd.py) of the leaves, in mpc_rollout's argument order"""
    n = L["v"].numel()
    f64 = dict(dtype=torch.float64, device=DEV)
    Tv = L["step_size"] * L["v"]
    one, zero = torch.ones(n, **f64), torch.zeros(n, **f64)
    rows = lambda x: x[:, None].expand(x.shape[0], n)
    w = L["weights"]
    return (torch.stack([one, Tv, zero, one]), torch.stack([zero, Tv, Tv / L["wheelbase"], -Tv / L["wheelbase"]]),
            torch.zeros(2, n, **f64), rows(w[0:2]), rows(w[2:4]), rows(L["lower"]), rows(L["upper"]), L["x0"],
            torch.stack([L["delta_y"], L["delta_phi"]]).repeat(H, 1))


GRAD_TO = ("weights", "v", "delta_y", "delta_phi", "step_size", "wheelbase", "x0")


@pytest.mark.parametrize("H,S,n,variant", [(10, 6, 300, "weights"), (4, 8, 300, "default")])
def test_autograd_forward_bytes_and_gradients_equal_mpc_rollout_on_the_expansion(H, S, n, variant):
    """Both backwards are tpc_mpc_rollout_backward on records that are the same bits, and both chain rules are the same
    torch graph: equality, bit for bit."""
    rng = np.random.default_rng(5)
    gc, gs = (torch.tensor(rng.standard_normal((S * 2, n)), device=DEV) for _ in range(2))
    with MpcSolver(horizon=H, device=0, algo="lane", **VARIANTS[variant]) as s:
        L = _leaves(H, n, variant)
        controls, states = mpc_rollout_compact(s, S, L["v"], L["delta_y"], L["delta_phi"], weights=L["weights"],
                                               step_size=L["step_size"], wheelbase=L["wheelbase"], lower=L["lower"],
                                               upper=L["upper"], x0=L["x0"], polish=(TOL, ROUNDS))
        raw = _loop(s, S, *[_np(L[k].detach()) for k in ("v", "delta_y", "delta_phi", "x0")], True, "solve")
        assert np.array_equal(bits(_np(controls.detach())), bits(raw["controls"]))
        assert np.array_equal(bits(_np(states.detach())), bits(raw["states"]))
        mine = torch.autograd.grad((controls * gc).sum() + (states * gs).sum(), [L[k] for k in GRAD_TO])
        R = _leaves(H, n, variant)
        rc, rs = mpc_rollout(s, S, *_expanded_tensors(R, H), polish=(TOL, ROUNDS), newton_first=True)
        assert np.array_equal(bits(_np(rc.detach())), bits(raw["controls"]))
        ref = torch.autograd.grad((rc * gc).sum() + (rs * gs).sum(), [R[k] for k in GRAD_TO])
    worst = 0.0
    for k, a, b in zip(GRAD_TO, mine, ref):
        a, b = _np(a), _np(b)
        rel = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
        worst = max(worst, rel)
        print(f"H={H} S={S} d{k}: largest difference relative to the largest entry {rel:.3e}")
        assert np.isfinite(b).all() and np.abs(b).max() > 0, k
        assert np.array_equal(bits(a), bits(b)), (k, rel)
    print(f"H={H} S={S}: carried by phase 1 {int((raw['first'] == S).sum())}/{n}, worst {worst:.3e}")


def _step(x):       # section 20's steps (tests/test_compact_grad_host.py)
    ax = np.abs(x)
    return np.where(ax > 0.1, 1e-6 * np.maximum(1.0, ax), 1e-4 * ax)


def test_autograd_matches_central_differences_in_the_log_weights():
    """d(mean states^2) / d(log weights) at (H, S, n) = (4, 6, 256) against central differences of the entry itself (tol
    1e-12, 32 rounds), with section 20's step sizes and keep rule: an instance counts when every run carried it to the
    end on one active set; at least 200 of 256 are kept and the norm-wise error is under 1e-5."""
    H, S, n = 4, 6, 256
    v, dy, dphi, x0, _ = _inputs(H, n, True, bad=False)
    p = capi.default_params(H)
    w0 = np.array([p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear])
    lo, hi = np.array(p.lower)[:, None], np.array(p.upper)[:, None]
    names = ("weight_y", "weight_phi", "weight_steering_front", "weight_steering_rear")
    with MpcSolver(horizon=H, device=0) as s:
        def run(w):
            c = _loop(s, S, v, dy, dphi, x0, True, "none", rounds=32, tol=1e-12, **dict(zip(names, w.tolist())))
            u = c["sequences"].reshape(S * H, 2, n)
            act = np.concatenate([u <= lo, u >= hi]).reshape(-1, n)
            return (c["states"] ** 2).mean(axis=0), c["first"] == S, act
        _, keep, act0 = run(w0)
        fd = np.zeros((4, n))
        for i in range(4):
            h = float(_step(w0[i]))
            vals = []
            for sign in (+1.0, -1.0):
                w = w0.copy()
                w[i] += sign * h
                loss, ok, act = run(w)
                keep = keep & ok & np.all(act == act0, axis=0)
                vals.append(loss)
            fd[i] = w0[i] * (vals[0] - vals[1]) / (2 * h)          # d / d log w = w d / dw
        kept = int(keep.sum())
        logw = torch.tensor(np.log(w0), requires_grad=True)
        controls, states = mpc_rollout_compact(s, S, _up(v, True), _up(dy, True), _up(dphi, True), weights=logw.exp(),
                                               x0=_up(x0, True), polish=(1e-12, 32))
        mask = torch.from_numpy(keep).to(DEV)
        ((states ** 2).mean(dim=0) * mask).sum().backward()
    got, want = logw.grad.numpy(), fd[:, keep].sum(axis=1)
    err = float(np.linalg.norm(got - want) / np.linalg.norm(got))
    print(f"kept {kept}/{n}; d/dlogw autograd {got.tolist()}, central differences {want.tolist()}, error {err:.3e}")
    assert kept >= 200
    assert err < 1e-5


# ---- 5. one large call

def test_large_call_at_the_reference_horizon():
    H, S, n = 4, 8, 262144
    v, dy, dphi = compact_inputs(H, n)
    with MpcSolver(horizon=H, device=0) as s:
        c, x, q, st, first = s.rollout_compact_exact(S, _up(v, True), _up(dy, True), _up(dphi, True), tol=TOL,
                                                     max_rounds=ROUNDS)
        torch.cuda.synchronize()
        flags = s.last_flags
    st, first = _np(st), _np(first)
    print(f"262144 x N=4 x 8 steps: unverified {int((first < S).sum())}, flags {flags:#x}, mean rounds at step 0 "
          f"{st[0].mean():.2f}, later {st[1:].mean():.2f}")
    assert flags == 0 and np.all(first == S) and np.all(st >= 0)
    assert np.all(np.isfinite(_np(c))) and np.all(np.isfinite(_np(x)))
