"""`-m gpu`: the hand-written coordinate-descent loop of the headline kernel (fp64, N = 20, csrc/mpc_ub_cd_asm.h) against the
CPU model of the LANE_FMA family (tests/model/), bit for bit and iteration for iteration -- around the phase boundaries
(the existing phase-boundary test runs at N = 10, where the compiled loop serves), with wavefronts that fail the screen
next to ones that pass it, a zero Q_diag, non-finite inputs and a partial last wavefront."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

H = 20


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def model():
    from tests.model.bindings import UbModel
    return UbModel()


def _solve(torch, v, dy, dphi, **kw):
    from trajectory_controller_amd import MpcSolver
    with MpcSolver(horizon=H, device=0, dtype="f64", algo="lane_fma", **kw) as s:
        tv, ty, tp = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, dy, dphi))
        f, r, it = s.solve_batch_compact(tv, ty, tp, want_iters=True)
        torch.cuda.synchronize()
        return f.cpu().numpy(), r.cpu().numpy(), it.cpu().numpy()


@pytest.mark.parametrize("smo", [0, 1, 2, 49, 50, 200])
@pytest.mark.parametrize("cap", [1, 3, 50, 51, 10000])
def test_cd_loop_phase_boundaries_n20(torch_cuda, model, smo, cap):
    from trajectory_controller_amd.synth import compact_inputs
    n = 700   # (not a multiple of 64: the last wavefront is partial)
    v, dy, dphi = compact_inputs(H, n, first=7000)
    mf, mr, mit, _ = model.solve_compact(H, v, dy, dphi, smo_iters=smo, max_iter=cap, nthreads=8)
    f, r, it = _solve(torch_cuda, v, dy, dphi, smo_iters=smo, max_iter=cap)
    assert np.array_equal(it, mit) and bits_equal(f, mf) and bits_equal(r, mr)


@pytest.mark.parametrize("weights", [None, (20.0, 0.0, 0.0005, 10.0)])
def test_cd_loop_mixed_screen_nonfinite_zero_qdiag_n20(torch_cuda, model, weights):
    """Non-finite inputs fail the screen: their wavefronts (0 and 14) take the compiled exact build, every other one the
    hand-written loop.  q1 = 0 makes Q_diag[H-1](0) = 0 (mpc.h:322's `continue`); v = 0 makes the whole gradient 0."""
    from trajectory_controller_amd.synth import compact_inputs
    n = 1000
    v, dy, dphi = (a.copy() for a in compact_inputs(H, n, first=3000))
    dy[5], v[14 * 64 + 3], dphi[14 * 64 + 9] = np.nan, np.inf, -np.inf
    v[300] = 0.0
    mkw = {} if weights is None else {"weights": weights}
    skw = {} if weights is None else dict(zip(("weight_y", "weight_phi", "weight_steering_front", "weight_steering_rear"), weights))
    for smo, cap in ((50, 10000), (3, 10000), (50, 51)):
        mf, mr, mit, _ = model.solve_compact(H, v, dy, dphi, smo_iters=smo, max_iter=cap, nthreads=8, fast_stop=None, **mkw)
        f, r, it = _solve(torch_cuda, v, dy, dphi, smo_iters=smo, max_iter=cap, **skw)
        assert np.array_equal(it, mit), (smo, cap)
        assert bits_equal(f, mf) and bits_equal(r, mr), (smo, cap)
        assert f[5] == 0 and r[5] == 0 and it[5] == 0
