"""GPU tests of the backward pass of the general form: the gfx950 kernel against the host path of the same entry (one
arithmetic header, so the same bits), against the dense reference (tests/model/mpc_grad_dense.py), and the torch
autograd functions (trajectory_controller_amd.autograd) against finite differences of the GPU solvers."""
import numpy as np
import pytest

from tests.conftest import bits_equal
from tests.model import mpc_grad_dense as dense
from trajectory_controller_amd import MpcSolver, mpc_compact, mpc_general
from trajectory_controller_amd.synth import compact_inputs, general_inputs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = dense.NAMES
CONVERGED = 20000   # iterations (of a cap of 200 000) within which an instance counts for a finite difference
KEY = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets")
OUTS = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "kkt_residual")


def _batch(I, H, n, seed):
    """SoA inputs of n instances and controls with many components on a bound (clipped noise), dL/du ~ N(0, 1)"""
    gi = general_inputs(H, n, I=I, seed=0x6AD1000 + 31 * H + I + seed)
    ins = [dense.soa(gi[k], n) for k in NAMES]
    rng = np.random.default_rng(seed + 17 * H + I)
    lo, hi = ins[5], ins[6]
    u = np.clip(rng.standard_normal((H * I, n)) * 0.3, np.tile(lo, (H, 1)), np.tile(hi, (H, 1)))
    g = rng.standard_normal((H * I, n))
    return ins, np.ascontiguousarray(u), g


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _gpu_backward(s, I, ins, u, g):
    out = s.solve_batch_general_backward(*[_dev(a) for a in ins], _dev(u), _dev(g), inputs=I)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, s.last_flags


@pytest.mark.parametrize("I,H,n", [(2, 20, 262144), (1, 1, 4099), (2, 1, 4099), (1, 3, 4099), (2, 7, 4099),
                                   (1, 20, 4099), (2, 33, 4099), (1, 47, 4099), (2, 64, 4099)])
def test_kernel_matches_host_path_bits(I, H, n):
    ins, u, g = _batch(I, H, n, 1)
    with MpcSolver(horizon=H, device=None) as hs:
        ref = hs.solve_batch_general_backward(*ins, u, g, inputs=I)
        assert hs.last_flags == 0
    with MpcSolver(horizon=H, device=0) as s:
        got, flags = _gpu_backward(s, I, ins, u, g)
    assert flags == 0
    for k in OUTS:
        assert bits_equal(got[k], ref[k]), k


def test_kernel_matches_dense_reference_host_memory_and_side_stream():
    I, H, n = 2, 20, 16
    th = dense.mixed_batch(I, H, n, seed=3)
    _, ustar, keep = dense.solved(I, H, th)
    g = np.random.default_rng(9).standard_normal((n, H, I))
    ins = [dense.soa(th[k], n) for k in NAMES]
    u, gs = dense.soa(ustar, n), dense.soa(g, n)
    with MpcSolver(horizon=H, device=0) as s:
        host_mem = s.solve_batch_general_backward(*ins, u, gs, inputs=I)       # numpy: HOST memory, staged
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            dev = s.solve_batch_general_backward(*[_dev(a) for a in ins], _dev(u), _dev(gs), inputs=I)
        side.synchronize()
        dev = {k: v.cpu().numpy() for k, v in dev.items()}
    with MpcSolver(horizon=H, device=None) as hs:
        cpu = hs.solve_batch_general_backward(*ins, u, gs, inputs=I)
    for k in OUTS:
        assert bits_equal(host_mem[k], cpu[k]) and bits_equal(dev[k], cpu[k]), k
    assert keep.sum() >= n // 2
    for i in np.flatnonzero(keep):
        ref, _, cond, _ = dense.instance(I, H, {k: th[k][i] for k in NAMES}, ustar[i], g[i])
        for k in NAMES:
            err = np.linalg.norm(dev[KEY[k]][:, i] - ref[k].ravel())
            assert err <= 1e-8 * np.linalg.norm(ref[k]) + 1e-300, (i, k, err, cond)


def _general_torch(H, I, n, seed):
    gi = general_inputs(H, n, I=I, seed=seed)
    return [_dev(dense.soa(gi[k], n)) for k in NAMES]


def _fd_check(solve, params, grads, g, keep_of, h_rel=1e-3, tol=1e-3, floor=0.01):
    """params: list of (name, tensor [rows, n]) the loss is differentiated by; grads: the autograd gradients of the
    same shapes.  Central differences, every instance perturbed at once (instances are independent); instances whose
    active set changes under any perturbation, or that take more than CONVERGED iterations in any solve, are left
    out: a slowly converging (ill-conditioned) instance stops at eps with an error that the step amplifies.
    Normwise per parameter over the kept instances.  (The solves stop at eps 1e-12, so the step is kept large enough for their residual to stay small
    against it; the tolerance is that of a central difference of that step.  The CPU tests hold the definition to
    1e-5 and the host path to 1e-8.)"""
    u0, act0 = solve(params)
    keep = keep_of(u0)
    fds = []
    for pi, (name, t) in enumerate(params):
        for r in range(t.shape[0]):
            h = h_rel * torch.clamp(t[r].abs(), min=floor)
            vals = []
            for sgn in (1.0, -1.0):
                pp = [(nm, tt.clone()) for nm, tt in params]
                pp[pi][1][r] += sgn * h
                u, act = solve(pp)
                keep &= keep_of(u) & torch.all(act == act0, dim=0)
                vals.append((u * g).sum(dim=0))
            fds.append((pi, r, (vals[0] - vals[1]) / (2 * h)))
    assert int(keep.sum()) >= keep.numel() // 2, int(keep.sum())
    for pi, r, fd in fds:
        ad = grads[pi][r]
        err = torch.linalg.norm((fd - ad)[keep]) / torch.linalg.norm(ad[keep]).clamp(min=1e-30)
        assert err < tol, (params[pi][0], r, float(err))


def test_mpc_general_forward_bits_and_gradients():
    I, H, n, eps, cap = 2, 10, 256, 1e-12, 200000
    ins = _general_torch(H, I, n, 0x6AD2000)
    with MpcSolver(horizon=H, device=0, eps=eps, max_iter=cap) as s:
        leaves = [t.clone().requires_grad_(True) for t in ins]
        u = mpc_general(s, *leaves)
        ctl = torch.zeros(H * I, n, dtype=torch.float64, device="cuda:0")
        u0 = s.solve_batch_general(*ins, controls=ctl, inputs=I)
        torch.cuda.synchronize()
        assert bits_equal(u.detach().cpu().numpy(), ctl.cpu().numpy())
        assert bits_equal(u[:I].detach().cpu().numpy(), u0.cpu().numpy())
        g = torch.randn(H * I, n, dtype=torch.float64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(5))
        grads = torch.autograd.grad((u * g).sum(), leaves)

        def solve(pp):
            c = torch.zeros(H * I, n, dtype=torch.float64, device="cuda:0")
            _, it = s.solve_batch_general(*[t for _, t in pp], controls=c, inputs=I, want_iters=True)
            lo, hi = pp[5][1].repeat(H, 1), pp[6][1].repeat(H, 1)
            solve.iters = it
            return c, (c <= lo) | (c >= hi)

        def keep_of(_):
            return solve.iters < CONVERGED
        params = [(k, t) for k, t in zip(NAMES, ins)]
        # every input but the bounds (no instance of this batch has a component on a bound in every perturbation
        # and the bound gradient is held to the dense reference by the CPU tests); targets: the first and last steps
        sel = [0, 1, 2, 3, 4, 7]
        tg = [0, 1, 2 * H - 2, 2 * H - 1]
        p_sel = [params[i] for i in sel] + [("targets", params[8][1][tg])]
        g_sel = [grads[i] for i in sel] + [grads[8][tg]]

        def solve_sel(pp):
            full = [t for _, t in params]
            for j, i in enumerate(sel):
                full[i] = pp[j][1]
            t8 = full[8].clone()
            t8[tg] = pp[-1][1]
            full[8] = t8
            return solve([(k, t) for k, t in zip(NAMES, full)])
        _fd_check(solve_sel, p_sel, g_sel, g, keep_of)


@pytest.mark.parametrize("H", [4, 20])
def test_mpc_compact_gradients_against_solve_batch_compact(H):
    n, eps, cap = 256, 1e-12, 200000
    v, dy, dphi = (_dev(a) for a in compact_inputs(H, n))
    w0 = (20.0, 7.0, 0.0005, 10.0)
    with MpcSolver(horizon=H, device=0, eps=eps, max_iter=cap) as s:
        tv, ty, tp = (t.clone().requires_grad_(True) for t in (v, dy, dphi))
        # the weights per instance ([4, n]): solve_batch_compact takes one set per batch, and a batch-wide step moves every
        # instance, so the finite difference of each instance's loss is that instance's derivative
        tw = torch.tensor(w0, dtype=torch.float64, device="cuda:0")[:, None].repeat(1, n).requires_grad_(True)
        front, rear = mpc_compact(s, tv, ty, tp, tw)
        gf = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(11))
        gr = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(12))
        amax = 22.0 * np.pi / 180.0

        def solve(args):
            vv, yy, pp, ww = args
            f, r, it = s.solve_batch_compact(vv, yy, pp, want_iters=True, weight_y=float(ww[0]), weight_phi=float(ww[1]),
                                             weight_steering_front=float(ww[2]), weight_steering_rear=float(ww[3]))
            solve.iters = it
            u = torch.stack([f, r])
            return u, (u <= -amax) | (u >= amax)

        # solve_batch_compact returns u0 only, so the stability check sees the active set of step 0 alone: the step is
        # kept small (1e-4 relative) so that it does not move a later step across a bound either
        # per-instance inputs: every instance perturbed at once
        g = torch.stack([gf, gr])
        grads = torch.autograd.grad((front * gf + rear * gr).sum(), [tv, ty, tp], retain_graph=True)
        wv = torch.tensor(w0, dtype=torch.float64)

        def solve_inst(pp):
            return solve([pp[0][1][0], pp[1][1][0], pp[2][1][0], wv])
        _fd_check(solve_inst, [("v", v[None].clone()), ("dy", dy[None].clone()), ("dphi", dphi[None].clone())],
                  [gg[None] for gg in grads], g, lambda _: solve.iters < CONVERGED, h_rel=1e-4)

        wv4 = torch.tensor(w0, dtype=torch.float64, device="cuda:0")[:, None].repeat(1, n)

        def solve_w(pp):
            return solve([v, dy, dphi, pp[0][1][:, 0]])
        _fd_check(solve_w, [("weights", wv4)], [torch.autograd.grad((front * gf + rear * gr).sum(), tw)[0]], g,
                  lambda _: solve.iters < CONVERGED, h_rel=1e-4, floor=1e-6)
