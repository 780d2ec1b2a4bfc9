"""GPU tests of the compact closed loop's backward pass (tpc_mpc_rollout_compact_exact_backward,
MpcSolver.rollout_compact_exact_backward, mpc_rollout_compact(backward="fused")): the device against the host-only
handle byte for byte per instance through the register kernels (H = 4, 5) and the workspace kernel, in HOST and DEVICE
memory and at the block thresholds; the device's deterministic batch sum of the shared parameters' gradients held to
the order of section 20 (cg.device_sum); the handle's other entries untouched by a call; the autograd switch against
the raw entries bit for bit and against the default route within section 20's bound for its two routes; one large
call."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import compact_grad_common as cg
from tests.model import compact_loop_common as cl
from tests.model import compact_loop_grad_common as lg
from tests.model.compact_loop_grad_common import ALL, NAMES, PER_INSTANCE, VARIANTS, bits
from trajectory_controller_amd import MpcSolver, capi, mpc_rollout_compact
from trajectory_controller_amd.synth import compact_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, ROUNDS = cl.TOL, cl.ROUNDS
KEYS = ("v", "dy", "dphi", "x0", "seq", "states", "st", "gc", "gs")


def _up(a, device=True):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if device else np.ascontiguousarray(a)


def _np(a):
    return None if a is None else np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)


@functools.lru_cache(maxsize=None)
def _case(H, n, S, variant="default", with_x0=False):
    """inputs, the host-only handle's forward records and backward, shared by the tests (never modified).  From 63
    instances on: one NaN speed (the forward stops it at step 0: status -1, zero rows) and one instance that the
    forward carried to the end whose status is set to -1 at its last step."""
    v, dy, dphi = (a.copy() for a in compact_inputs(H, n))
    if n >= 63:
        v[5] = np.nan
    x0 = cl.start_states(H, n) if with_x0 else None
    gc, gs = lg.grads_in(S, n, 17 + H + S)
    with MpcSolver(horizon=H, device=None, **VARIANTS[variant]) as s:
        r = cl.loop(s, S, v, dy, dphi, x0)
        st = r["status"].copy()
        if n >= 63:
            st[S - 1, np.flatnonzero((st >= 0).all(axis=0))[7]] = -1
        want = s.rollout_compact_exact_backward(S, v, dy, dphi, x0, sequences=r["sequences"], states=r["states"],
                                                status=st, grad_controls=gc, grad_states=gs, want=ALL)
        flags = s.last_flags
    return dict(v=v, dy=dy, dphi=dphi, x0=x0, seq=r["sequences"], states=r["states"], st=st, gc=gc, gs=gs, S=S,
                want=want, flags=flags)


def _backward(s, c, device, want=ALL, status=True):
    a = {k: _up(c[k], device) for k in KEYS}
    got = s.rollout_compact_exact_backward(c["S"], a["v"], a["dy"], a["dphi"], a["x0"], sequences=a["seq"],
                                           states=a["states"], status=a["st"] if status else None,
                                           grad_controls=a["gc"], grad_states=a["gs"], want=want)
    if device:
        torch.cuda.synchronize()
    return {k: _np(x) for k, x in got.items()}, s.last_flags


# ---- 1. device against host: H = 4, 5 the register kernels, 1 / 7 / 20 / 64 the workspace kernel

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("with_x0", [False, True], ids=["x0=null", "x0"])
@pytest.mark.parametrize("variant", ["default", "weights", "offset"])
@pytest.mark.parametrize("H", [4, 5, 1, 7, 20, 64])
def test_device_equals_host_only_handle_bytes(H, variant, with_x0, device):
    with MpcSolver(horizon=H, device=0, **VARIANTS[variant]) as s:
        for n in (1, 63, 65, 300):
            for S in (1, 5):
                c = _case(H, n, S, variant, with_x0)
                got, flags = _backward(s, c, device)
                for k in PER_INSTANCE:
                    assert got[k].tobytes() == c["want"][k].tobytes(), (n, S, k)
                assert flags == c["flags"] == (capi.FLAG_NONFINITE if n >= 63 else 0), (n, S)
                excluded = (c["st"] < 0).any(axis=0)
                assert n < 63 or excluded.sum() >= 2
                for k in PER_INSTANCE:
                    assert not bits(got[k][..., excluded]).any(), (n, S, k)
                rows = got["params_rows"]
                assert got["params"].tobytes() == cg.device_sum(rows).tobytes(), (n, S)
                assert np.all(np.abs(got["params"] - c["want"]["params"]) <= 2 * cg.fsum_bound(rows)), (n, S)


# the launcher's block is the largest of 256, 128, 64 that gives every CU a block: 32 641 lanes are the first batch on
# blocks of 128, 65 280 the last on 128 and 65 281 the first on 256
@pytest.mark.parametrize("H,n", [(4, 32641), (4, 65280), (4, 65281), (7, 65281)])
def test_block_thresholds(H, n):
    c = _case(H, n, 2, "default", True)
    with MpcSolver(horizon=H, device=0) as s:
        got, flags = _backward(s, c, True)
    for k in PER_INSTANCE:
        assert got[k].shape[-1] == n and got[k].tobytes() == c["want"][k].tobytes(), k
    assert flags == c["flags"] == capi.FLAG_NONFINITE
    rows = got["params_rows"]
    assert rows[:, -1].any(), "the last instance's row is zero: its lane shows no work"
    assert got["params"].tobytes() == cg.device_sum(rows).tobytes()
    assert np.all(np.abs(got["params"] - cg.fsum_rows(rows)) <= cg.fsum_bound(rows))


# ---- 2. dparams on the device: no floating-point atomics, section 20's order

@pytest.mark.parametrize("H", [4, 20])
def test_dparams_is_deterministic_and_in_the_documented_order(H):
    with MpcSolver(horizon=H, device=0) as s:
        for n in (1, 65, 300, 4096):
            c = _case(H, n, 5, "default", True)
            got, _ = _backward(s, c, True)
            rows = got["params_rows"]
            diff = np.abs(got["params"] - cg.fsum_rows(rows))
            print(f"H={H} n={n}: max |dparams - fsum| / bound "
                  f"{np.max(diff / np.maximum(cg.fsum_bound(rows), 1e-300)):.3f}")
            assert np.all(diff <= cg.fsum_bound(rows)), (n, diff, cg.fsum_bound(rows))
            assert got["params"].tobytes() == cg.device_sum(rows).tobytes(), n     # the documented order, to the bit
            again, _ = _backward(s, c, True)
            assert again["params"].tobytes() == got["params"].tobytes(), n
            with torch.cuda.stream(torch.cuda.Stream(device=DEV)):
                other, _ = _backward(s, c, True)
            assert other["params"].tobytes() == got["params"].tobytes(), n
            alone, _ = _backward(s, c, True, want=("params",))       # the per-instance outputs not requested
            assert set(alone) == {"params"} and alone["params"].tobytes() == got["params"].tobytes(), n
            staged, _ = _backward(s, c, False, want=("params",))     # HOST arrays: the same launches
            assert staged["params"].tobytes() == got["params"].tobytes(), n


# ---- 3. the handle's other entries: the gradient workspace is shared

def test_other_entries_return_the_same_bytes_around_a_backward_call():
    H, n, S = 10, 300, 4
    c = _case(H, n, S, "default", True)
    v, dy, dphi = compact_inputs(H, n)
    tv, ty, tp, tx = (_up(a) for a in (v, dy, dphi, c["x0"]))
    th = cl.expanded(capi.default_params(H), H, v, dy, dphi, c["x0"])
    ins = [_up(th[k]) for k in NAMES]
    gc, gs = _up(c["gc"]), _up(c["gs"])

    def others(s):
        fwd = s.rollout_compact_exact(S, tv, ty, tp, tx, tol=TOL, max_rounds=ROUNDS)
        out = [a for a in fwd if a is not None]
        one = s.solve_batch_compact_exact(tv, ty, tp, tol=TOL, max_rounds=ROUNDS, want_sequence=True)
        out += list(s.solve_batch_compact_exact_backward(tv, ty, tp, one[2], grad_front=gc[0], grad_rear=gc[1],
                                                         status=one[3], want=cg.PER_INSTANCE + ("params",)).values())
        out += list(s.rollout_backward(S, *ins, None, sequences=fwd[2], states=fwd[1], grad_controls=gc,
                                       grad_states=gs, inputs=2).values())
        torch.cuda.synchronize()
        return [_np(a).tobytes() for a in out]

    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        before = others(s)
        got, _ = _backward(s, c, True)
        assert others(s) == before
        again, _ = _backward(s, c, True)
        for k in ALL:
            assert again[k].tobytes() == got[k].tobytes(), k


# ---- 4. autograd

def _leaves(H, n, variant):
    v, dy, dphi = compact_inputs(H, n)
    x0 = cl.start_states(H, n)
    p = capi.default_params(H, **VARIANTS[variant])
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV, requires_grad=True)
    return dict(v=t(v), delta_y=t(dy), delta_phi=t(dphi), x0=t(x0),
                weights=t([p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear]),
                step_size=t(p.step_size), wheelbase=t(p.wheelbase), lower=t(list(p.lower)), upper=t(list(p.upper)))


def _compact(s, S, L, **kw):
    return mpc_rollout_compact(s, S, L["v"], L["delta_y"], L["delta_phi"], weights=L["weights"],
                               step_size=L["step_size"], wheelbase=L["wheelbase"], lower=L["lower"], upper=L["upper"],
                               x0=L["x0"], polish=(TOL, ROUNDS), **kw)


GRAD_TO = ("weights", "v", "delta_y", "delta_phi", "step_size", "wheelbase", "x0")
AUTOGRAD_CASES = [(10, 6, 300, "weights"), (4, 8, 300, "default")]


@pytest.mark.parametrize("H,S,n,variant", AUTOGRAD_CASES)
def test_fused_autograd_equals_the_raw_entries(H, S, n, variant):
    rng = np.random.default_rng(5)
    gc, gs = (torch.tensor(rng.standard_normal((S * 2, n)), device=DEV) for _ in range(2))
    leaves = GRAD_TO + ("lower", "upper")
    with MpcSolver(horizon=H, device=0, algo="lane", **VARIANTS[variant]) as s:
        L = _leaves(H, n, variant)
        controls, states = _compact(s, S, L, backward="fused")
        ins = [L[k].detach() for k in ("v", "delta_y", "delta_phi", "x0")]
        rc, rs, rq, _, _ = s.rollout_compact_exact(S, *ins, tol=TOL, max_rounds=ROUNDS)
        torch.cuda.synchronize()
        assert np.array_equal(bits(_np(controls.detach())), bits(_np(rc)))
        assert np.array_equal(bits(_np(states.detach())), bits(_np(rs)))
        mine = dict(zip(leaves, torch.autograd.grad((controls * gc).sum() + (states * gs).sum(),
                                                    [L[k] for k in leaves])))
        raw = s.rollout_compact_exact_backward(S, *ins, sequences=rq, states=rs, grad_controls=gc, grad_states=gs)
        torch.cuda.synchronize()
        # only the outputs someone needs: nothing to differentiate, no call; v alone, the same bytes
        L2 = {k: t.detach() for k, t in L.items()}
        L2["v"] = L2["v"].clone().requires_grad_()
        c2, x2 = _compact(s, S, L2, backward="fused")
        (only_v,) = torch.autograd.grad((c2 * gc).sum() + (x2 * gs).sum(), [L2["v"]])
        torch.cuda.synchronize()
    for k in ("v", "delta_y", "delta_phi", "x0"):
        assert _np(mine[k]).tobytes() == _np(raw[k]).tobytes(), k
    par = _np(raw["params"])
    for k, sl in (("weights", slice(0, 4)), ("step_size", 4), ("wheelbase", 5), ("lower", slice(6, 8)),
                  ("upper", slice(8, 10))):
        assert mine[k].shape == L[k].shape and mine[k].device == L[k].device
        assert _np(mine[k]).tobytes() == np.ascontiguousarray(par[sl]).tobytes(), k
    assert _np(only_v).tobytes() == _np(raw["v"]).tobytes()


@pytest.mark.parametrize("H,S,n,variant", AUTOGRAD_CASES)
def test_fused_autograd_agrees_with_the_default_route(H, S, n, variant):
    """Both routes take the same derivative at the same records; they differ in the order of the sums over the batch
    and over the targets and in where the chain rule is rounded.  The bound is 1e-8 norm-wise per leaf, section 20's
    bound for its two routes.  Measured worst: 3.5e-16."""
    rng = np.random.default_rng(5)
    gc, gs = (torch.tensor(rng.standard_normal((S * 2, n)), device=DEV) for _ in range(2))
    grads = {}
    with MpcSolver(horizon=H, device=0, algo="lane", **VARIANTS[variant]) as s:
        for route in ("fused", "expanded"):
            L = _leaves(H, n, variant)
            controls, states = _compact(s, S, L, backward=route)
            grads[route] = [_np(g) for g in torch.autograd.grad((controls * gc).sum() + (states * gs).sum(),
                                                                [L[k] for k in GRAD_TO])]
        with pytest.raises(ValueError):
            _compact(s, S, _leaves(H, n, variant), backward="nonsense")
    worst = 0.0
    for k, a, b in zip(GRAD_TO, grads["fused"], grads["expanded"]):
        assert np.isfinite(b).all() and np.abs(b).max() > 0, k
        rel = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print(f"H={H} S={S} d{k}: norm-wise relative difference {rel:.3e}")
        worst = max(worst, rel)
    print(f"H={H} S={S} {variant}: worst {worst:.3e}")
    assert worst <= 1e-8


# ---- 5. one large call

def test_large_call_at_the_reference_horizon():
    H, S, n = 4, 8, 262144
    v, dy, dphi = compact_inputs(H, n)
    gc, gs = lg.grads_in(S, n, 2)
    with MpcSolver(horizon=H, device=0) as s:
        tv, ty, tp = _up(v), _up(dy), _up(dphi)
        c, x, q, st, _ = s.rollout_compact_exact(S, tv, ty, tp, tol=TOL, max_rounds=ROUNDS)
        got = s.rollout_compact_exact_backward(S, tv, ty, tp, sequences=q, states=x, status=st,
                                               grad_controls=_up(gc), grad_states=_up(gs), want=ALL)
        torch.cuda.synchronize()
        flags = s.last_flags
    print(f"262144 x N=4 x 8 steps: flags {flags:#x}, dparams {_np(got['params']).tolist()}")
    assert flags == 0
    for k in ALL:
        assert np.all(np.isfinite(_np(got[k]))), k
    rows = _np(got["params_rows"])
    assert _np(got["params"]).tobytes() == cg.device_sum(rows).tobytes()     # 256-lane blocks, 1024 partials
