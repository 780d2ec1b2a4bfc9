"""`-m gpu` tests of the table-predicted queue key of LANE_FMA at fp64, N = 20 (csrc/mpc_queue_key.h, ub_cd_kernel in
csrc/mpc_ub.h): the key decides which lane solves which instance when, and nothing else.  4 096 + 37 instances: a partial last
wavefront, 65 wavefronts of the persistent grid with one instance per lane.  Where lanes see more than one instance -- the
grid pinned to one wavefront, every lane refilled four or five times, the table's key, lambda's and hints in both orders
against the CPU model -- is tests/test_refill_gpu.py (test_refill_lane_fma_queue_order_changes_nothing_n20).
"""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

H, N = 20, 4096 + 37


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def batch():
    from trajectory_controller_amd.synth import compact_inputs
    return compact_inputs(H, N, first=300000)


@pytest.fixture(scope="module")
def edge_batch(batch):
    """the same batch with every 97th instance replaced: speeds 0.05 and 6.0 (below and above the table's range), targets
    outside its box, non-finite speeds and targets"""
    v, dy, dphi = (a.copy() for a in batch)
    edges = [(0.05, 0.1, 0.1), (6.0, -0.2, 0.3), (1.0, 2.0, 0.1), (2.0, -0.1, -1.5), (0.05, -2.0, 1.5), (6.0, 0.9, -0.9),
             (np.nan, 0.1, 0.1), (1.0, np.inf, 0.0), (1.0, 0.0, -np.inf), (np.inf, 0.0, 0.0), (2.0, np.nan, np.nan)]
    for j, k in enumerate(range(5, N, 97)):
        v[k], dy[k], dphi[k] = edges[j % len(edges)]
    return v, dy, dphi


def _solver(**kw):
    from trajectory_controller_amd import MpcSolver
    return MpcSolver(horizon=H, device=0, dtype="f64", algo="lane_fma", **kw)


def _run(torch, s, b):
    tv, ty, tp = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in b)
    f, r, it = s.solve_batch_compact(tv, ty, tp, want_iters=True)
    torch.cuda.synchronize()
    return f.cpu().numpy(), r.cpu().numpy(), it.cpu().numpy()


def _same(a, b):
    return bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_key_on_off_same_bits_and_model(torch_cuda, batch):
    from tests.model.bindings import UbModel
    mf, mr, mit, _ = UbModel().solve_compact(H, *batch, nthreads=8)
    with _solver() as s:
        on = _run(torch_cuda, s, batch)
        assert s.last_queue_key() == "table"
        s.set_queue_key(False)
        off = _run(torch_cuda, s, batch)
        assert s.last_queue_key() == "lambda"
        s.set_queue_key(True)
        again = _run(torch_cuda, s, batch)
        assert s.last_queue_key() == "table"
    assert _same(on, off) and _same(on, again)
    assert np.array_equal(on[2], mit)
    assert bits_equal(on[0], mf) and bits_equal(on[1], mr)


def test_other_parameters_keep_lambda(torch_cuda, batch):
    """the table speaks about ONE parameter set: any other weight, bound, eps or cap reports (and runs) the lambda key"""
    small = tuple(a[:300] for a in batch)
    with _solver(weight_y=21.0) as s:
        _run(torch_cuda, s, small)
        assert s.last_queue_key() == "lambda"
    with _solver() as s:
        for over in (dict(weight_steering_rear=9.0), dict(eps=0.02), dict(max_iter=9999), dict(smo_iters=49), dict(step_size=0.05),
                     dict(wheelbase=0.25), dict(upper=(0.3, 0.3)), dict(lower=(-0.3, -0.38397243543875248))):
            tv, ty, tp = (torch_cuda.from_numpy(a).to("cuda:0") for a in small)
            s.solve_batch_compact(tv, ty, tp, **over)
            assert s.last_queue_key() == "lambda", over
        _run(torch_cuda, s, small)
        assert s.last_queue_key() == "table"
    for kw in (dict(algo="lane"), dict(algo="group"), dict(dtype="f32"), dict(horizon=10)):
        from trajectory_controller_amd import MpcSolver
        cfg = dict(horizon=H, device=0, dtype="f64", algo="lane_fma")
        cfg.update(kw)
        with MpcSolver(**cfg) as s:
            dt = torch_cuda.float32 if cfg["dtype"] == "f32" else torch_cuda.float64
            tv, ty, tp = (torch_cuda.from_numpy(a).to("cuda:0", dtype=dt) for a in small)
            s.solve_batch_compact(tv, ty, tp)
            assert s.last_queue_key() == "lambda", kw


def test_work_hint_wins(torch_cuda, batch):
    with _solver() as s:
        base = _run(torch_cuda, s, batch)
        s.set_work_hint(np.maximum(base[2], 1).astype(np.int32))
        hinted = _run(torch_cuda, s, batch)
        assert s.last_queue_key() == "hint"
        wi_hint, _ = s.last_lane_stats()
        after = _run(torch_cuda, s, batch)          # (a hint lasts one solve)
        assert s.last_queue_key() == "table"
        wi_table, _ = s.last_lane_stats()
    assert _same(base, hinted) and _same(base, after)
    # the exact counts as the hint order the queue better than any prediction: were the hint ignored, the two would agree
    print(f"wave iterations: exact-count hint {wi_hint}, table {wi_table}")
    assert wi_hint < wi_table


def test_edge_inputs_same_results_fewer_wave_iterations(torch_cuda, edge_batch):
    """speeds and targets outside the table's box and non-finite inputs among ordinary instances: same bits with the key on
    and off, and the order the table gives costs no more wave iterations than lambda's.  At this size every lane gets one
    instance, so a wavefront costs its longest: simulated on the model's counts over the arbitrary orders inside the bins,
    76 381 ... 76 406 sums of per-wavefront maxima against 79 464 ... 79 597 (NOTEBOOK round 7: with speeds above the box
    reading its face it was 76 256 ... 80 381, and 80 409 against 79 517 measured)"""
    with _solver() as s:
        on = _run(torch_cuda, s, edge_batch)
        assert s.last_queue_key() == "table"
        wi_on, _ = s.last_lane_stats()
        s.set_queue_key(False)
        off = _run(torch_cuda, s, edge_batch)
        wi_off, _ = s.last_lane_stats()
    assert _same(on, off)
    print(f"wave iterations: table {wi_on}, lambda {wi_off}")
    assert 0 < wi_on <= wi_off
