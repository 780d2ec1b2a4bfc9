"""GPU tests of the polish of the general form: the gfx950 kernel against the host path of the same entry (one
arithmetic header, so the same bits) through the numpy and the CUDA-tensor entry, the autograd functions with
polish=True against finite differences of the GPU solver, and the flagship batch once."""
import numpy as np
import pytest

from oracle.bindings import Oracle
from tests.conftest import bits_equal
from tests.model import mpc_grad_dense as dense
from trajectory_controller_amd import MpcSolver, capi, mpc_general
from trajectory_controller_amd.synth import general_inputs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = dense.NAMES
TOL, ROUNDS = 1e-10, 8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _inputs(kind, I, H, n):
    """SoA inputs and the oracle's controls at dlib's eps 0.01, [H*I, n]"""
    if kind == "general":
        gi = general_inputs(H, n, I=I, seed=5)
        th = {k: gi[k] for k in NAMES}
    else:
        th = dense.mixed_batch(I, H, n)
    _, ctl, _ = Oracle().solve_general(I, H, *[th[k] for k in NAMES], eps=0.01)
    return [dense.soa(th[k], n) for k in NAMES], dense.soa(ctl, n)


@pytest.mark.parametrize("kind", ["general", "mixed"])
@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H", [4, 10, 20, 40, 64])
def test_kernel_matches_host_path_bits(kind, I, H):
    n = 300
    ins, ctl = _inputs(kind, I, H, n)
    with MpcSolver(horizon=H, device=None) as hs:
        ref = hs.polish_batch_general(*ins, ctl.copy(), tol=TOL, max_rounds=ROUNDS, inputs=I)
        ref_flags = hs.last_flags
    with MpcSolver(horizon=H, device=0) as s:
        staged = s.polish_batch_general(*ins, ctl.copy(), tol=TOL, max_rounds=ROUNDS, inputs=I)   # numpy: HOST, staged
        staged_flags = s.last_flags
        dev = s.polish_batch_general(*[_dev(a) for a in ins], _dev(ctl), tol=TOL, max_rounds=ROUNDS, inputs=I)
        torch.cuda.synchronize()
        dev_flags = s.last_flags
        dev = [t.cpu().numpy() for t in dev]
    assert staged_flags == ref_flags and dev_flags == ref_flags
    for name, r, a, b in zip(("controls", "status", "residual_in", "residual_out"), ref, staged, dev):
        assert bits_equal(a, r), (name, "numpy entry")
        assert bits_equal(b, r), (name, "tensor entry")
    assert np.array_equal(ref[0][:, ref[1] < 0], ctl[:, ref[1] < 0])


def test_mpc_general_polish_gradients_and_default_bits():
    """eps 0.01 + polish, differentiated, against central differences of the GPU solver at eps 1e-12: the tolerances
    of tests/test_grad_gpu.py's eps-1e-12 case (its _fd_check: step 1e-3 relative, 1e-3 normwise)."""
    from tests.test_grad_gpu import CONVERGED, _fd_check, _general_torch
    I, H, n, eps, cap = 2, 10, 256, 1e-12, 200000
    ins = _general_torch(H, I, n, 0x6AD2000)
    with MpcSolver(horizon=H, device=0, eps=eps, max_iter=cap) as s:
        # polish=False is the function without the keyword, byte for byte
        plain = mpc_general(s, *ins, eps=0.01)
        off = mpc_general(s, *ins, eps=0.01, polish=False)
        torch.cuda.synchronize()
        assert bits_equal(plain.cpu().numpy(), off.cpu().numpy())

        leaves = [t.clone().requires_grad_(True) for t in ins]
        u = mpc_general(s, *leaves, eps=0.01, polish=True)
        assert not bits_equal(u.detach().cpu().numpy(), plain.cpu().numpy())
        g = torch.randn(H * I, n, dtype=torch.float64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(5))
        grads = torch.autograd.grad((u * g).sum(), leaves)
        lo, hi = ins[5].repeat(H, 1), ins[6].repeat(H, 1)
        act_polished = (u.detach() <= lo) | (u.detach() >= hi)

        def solve(pp):
            c = torch.zeros(H * I, n, dtype=torch.float64, device="cuda:0")
            _, it = s.solve_batch_general(*[t for _, t in pp], controls=c, inputs=I, want_iters=True)
            l, h = pp[5][1].repeat(H, 1), pp[6][1].repeat(H, 1)
            solve.iters = it
            return c, (c <= l) | (c >= h)

        _, act_ref = solve(list(zip(NAMES, ins)))
        same_set = torch.all(act_polished == act_ref, dim=0)

        def keep_of(_):
            return (solve.iters < CONVERGED) & same_set
        params = [(k, t) for k, t in zip(NAMES, ins)]
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


def test_flagship_batch_once():
    I, H, n = 2, 20, 262144
    gi = general_inputs(H, n, I=I, seed=5)
    ins = [_dev(dense.soa(gi[k], n)) for k in NAMES]
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        ctl = torch.zeros(H * I, n, dtype=torch.float64, device="cuda:0")
        s.solve_batch_general(*ins, controls=ctl, inputs=I, eps=0.01)
        before = ctl.clone()
        _, st, rin, rout = s.polish_batch_general(*ins, ctl, tol=TOL, max_rounds=ROUNDS, inputs=I)
        torch.cuda.synchronize()
        flags = s.last_flags
    ok = st >= 0
    print(f"262144 x N=20: polished {int(ok.sum())}, status histogram {torch.bincount(st[ok]).tolist()}, "
          f"max residual in {float(rin.max()):.3e}")
    assert bool(torch.all(rout[ok] <= TOL)) and bool(torch.all(rout <= rin))
    assert bits_equal(ctl[:, ~ok].cpu().numpy(), before[:, ~ok].cpu().numpy())
    assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((~ok).any())
    assert int(ok.sum()) >= 0.99 * n
