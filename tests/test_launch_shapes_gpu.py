"""GPU tests of the launch shapes of the one-lane-per-instance fp64 kernels.  rollout_grad_block() gives blocks of 64
lanes below 32641 lanes, of 128 from 32641 and of 256 from 65281, and every launcher of the family uses it (the tangent
kernels with lanes = K * n).  Here each launcher runs at 32641 lanes (the first grid of 128-lane blocks, one live lane
in the last block), 65280 (the last one, every block full) and 65281 (the first grid of 256-lane blocks, one live lane
in the last block), DEVICE memory, with the smallest problem that still runs every loop, and must return the host-only
handle's bits; the last instance's column must show that its lane did work.  (With K = 3 directions the lane count is
3 n, which meets only 65280 exactly: see CASES.)

What is covered, and how:
  against the host-only handle's bits (LAUNCHERS, test_device_equals_host_only_handle_bits_at_the_block_thresholds)
    polish, backward, forward / forward_k1    the single general-form solve's polish, adjoint and tangent kernels
    exact_reg / exact_ws                      the cold exact compact forward, H = 4 (registers) and 7 (workspace)
    exact_rows_reg / exact_rows_ws            the same with per-instance parameters
    compact_backward_reg / _ws,               both compact backward entries without "params": the per-instance outputs.
    compact_rows_backward_reg / _ws           With "params" (block_partials and the reduce kernel) the same kernels
                                              are held to these bytes and to cg.device_sum at these counts and four
                                              more in tests/test_compact_grad_gpu.py and tests/test_compact_rows_gpu.py
    newton, rollout_backward, rollout_forward the Newton-first closed loop and the derivatives on its recorded loop
    plant_newton, plant_backward,             rollout_plant_newton_kernel, rollout_plant_bwd_kernel and
    plant_forward                             rollout_plant_fwd_kernel (K = 1), on the host-only plant loop's record
  against the loop composed from the public entries (test_fused_polished_loops_...): rollout_polish_step_kernel and
    rollout_plant_polish_step_kernel, which have no host path
  elsewhere: the warm-started exact compact forward, tests/test_compact_warm_gpu.py::test_launch_shapes."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.bindings import Oracle
from tests import test_compact_grad_gpu as compact_grad_gpu
from tests import test_compact_rows_gpu as compact_rows_gpu
from tests import test_rollout_plant_gpu as plant_gpu
from tests import test_rollout_polish_gpu as polish_gpu
from tests.model import compact_grad_common as cg
from tests.model import compact_rows_common as cr
from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.model import mpc_rollout_tangent_dense as td
from tests.model.compact_exact_common import ROUNDS as EXACT_ROUNDS, TOL
from tests.test_rollout_newton_host import soa_inputs
from tests.test_rollout_plant_host import make_plant
from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import compact_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = dense.NAMES
LANES = [32641, 65280, 65281]
ROUNDS = 8


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)


def _model(I, H, n):
    """mixed_batch's SoA arrays and controls in the box with many components on a bound (clipped noise)"""
    th = dense.mixed_batch(I, H, n)
    ins = [dense.soa(th[k], n) for k in NAMES]
    rng = np.random.default_rng(3 + 17 * H + I)
    u = np.clip(rng.standard_normal((H * I, n)) * 0.3, np.tile(ins[5], (H, 1)), np.tile(ins[6], (H, 1)))
    return th, ins, np.ascontiguousarray(u), rng


# Each launcher: data(n) -> the call's numpy inputs, run(s, data, conv) -> the outputs in a fixed order (conv moves an
# array to the memory s works on), live(outputs) -> the last instance's column shows work done

def _polish_data(n):
    th, ins, _, _ = _model(2, 4, n)
    _, ctl, _ = Oracle().solve_general(2, 4, *[th[k] for k in NAMES], eps=0.01)
    return ins, dense.soa(ctl, n)


def _polish_run(s, d, conv):
    ins, u = d
    c = conv(u.copy())      # updated in place
    _, st, ri, ro = s.polish_batch_general(*[conv(a) for a in ins], c, tol=TOL, max_rounds=ROUNDS, inputs=2)
    return [c, st, ri, ro]


def _backward_data(n):
    _, ins, u, rng = _model(1, 2, n)
    return ins, u, rng.standard_normal(u.shape)


def _backward_run(s, d, conv):
    ins, u, g = d
    out = s.solve_batch_general_backward(*[conv(a) for a in ins], conv(u), conv(g), inputs=1)
    return [out[k] for k in s.GRAD_NAMES]


def _forward_data(n, K=3):
    _, ins, u, _ = _model(2, 2, n)
    return ins, u, td.soa_tangents(td.random_tangents(2, 2, 1, n, 12, with_nlt=False, K=K), n)


def _forward_run(s, d, conv):
    ins, u, tan = d
    return [s.solve_batch_general_forward(*[conv(a) for a in ins], conv(u), {k: conv(v) for k, v in tan.items()},
                                          inputs=2)]


def _exact_run(s, d, conv):
    """d: (v, delta_y, delta_phi) the shared-parameter kernels, with a fourth array [10, n] the rows kernels"""
    out = s.solve_batch_compact_exact(*[conv(a) for a in d[:3]], tol=TOL, max_rounds=EXACT_ROUNDS, fallback="none",
                                      want_sequence=True, want_residuals=True,
                                      params_rows=conv(d[3]) if len(d) > 3 else None)
    assert out[4] is None       # fell_back: not with fallback="none"
    return [a for a in out if a is not None]


def _compact_backward_run(s, c, conv):
    """c: the _case of tests/test_compact_grad_gpu.py or tests/test_compact_rows_gpu.py (the host-only handle's forward
    sequence, one NaN speed, one verified instance excluded).  "params" is not requested: a lane past the batch leaves
    at once.  With it the same kernels run in those files' seam tests, at these lane counts among others."""
    kw = {"params_rows": conv(c["rows"])} if "rows" in c else {}
    out = s.solve_batch_compact_exact_backward(*[conv(c[k]) for k in ("v", "dy", "dphi", "seq", "gf", "gr", "gs")],
                                               status=conv(c["st"]), want=cg.PER_INSTANCE, **kw)
    return [out[k] for k in cg.PER_INSTANCE]


NEWTON = (2, 4, 2)      # I, H, S


def _newton_data(n):
    I, H, S = NEWTON
    th, nlt = rd.batch(I, H, S, n, seed=2)
    return soa_inputs(th, nlt, n)


def _newton_run(s, d, conv):
    I, H, S = NEWTON
    ins, nl = d
    return list(s.rollout_newton(S, *[conv(a) for a in ins], conv(nl), inputs=I, tol=TOL, max_rounds=ROUNDS,
                                 fallback="none", want_iters=True))


def _recorded(n):
    """the host rollout_newton's sequences and states, and the seeds of the loss"""
    (ins, nl), (out, _) = _data("newton", n), _host("newton", n)
    return ins, nl, out[2], out[1], np.random.default_rng(21)


def _rollout_backward_data(n):
    I, H, S = NEWTON
    ins, nl, q, x, rng = _recorded(n)
    return ins, nl, q, x, rng.standard_normal((S * I, n)), rng.standard_normal((2 * S, n))


def _rollout_backward_run(s, d, conv):
    I, H, S = NEWTON
    ins, nl, q, x, gu, gx = d
    out = s.rollout_backward(S, *[conv(a) for a in ins], conv(nl), sequences=conv(q), states=conv(x),
                             grad_controls=conv(gu), grad_states=conv(gx), inputs=I)
    return [out[k] for k in s.ROLLOUT_GRAD_NAMES]


def _rollout_forward_data(n):
    I, H, S = NEWTON
    ins, nl, q, x, _ = _recorded(n)
    return ins, nl, q, x, td.soa_tangents(td.random_tangents(I, H, S, n, 22, K=1), n)


def _rollout_forward_run(s, d, conv):
    I, H, S = NEWTON
    ins, nl, q, x, tan = d
    return list(s.rollout_forward(S, *[conv(a) for a in ins], conv(nl), sequences=conv(q), states=conv(x),
                                  tangents={k: conv(v) for k, v in tan.items()}, inputs=I))


def _plant_kw(plant, dist, conv):
    return dict(plant=tuple(conv(a) for a in plant), disturbance=conv(dist))


def _plant_newton_data(n):
    """the Newton loop's problem against a plant and a disturbance of its own (make_plant)"""
    ins, nl = _data("newton", n)
    return ins, nl, make_plant(ins, NEWTON[0], NEWTON[2])


def _plant_newton_run(s, d, conv):
    I, H, S = NEWTON
    ins, nl, (plant, dist) = d
    return list(s.rollout_newton(S, *[conv(a) for a in ins], conv(nl), inputs=I, tol=TOL, max_rounds=ROUNDS,
                                 fallback="none", want_iters=True, **_plant_kw(plant, dist, conv)))


def _plant_recorded(n):
    """the host plant loop's sequences and states"""
    (ins, nl, (plant, dist)), (out, _) = _data("plant_newton", n), _host("plant_newton", n)
    return ins, nl, plant, dist, out[2], out[1]


def _plant_backward_data(n):
    I, H, S = NEWTON
    rng = np.random.default_rng(23)
    return _plant_recorded(n) + (rng.standard_normal((S * I, n)), rng.standard_normal((2 * S, n)))


def _plant_backward_run(s, d, conv):
    I, H, S = NEWTON
    ins, nl, plant, dist, q, x, gu, gx = d
    out = s.rollout_backward(S, *[conv(a) for a in ins], conv(nl), sequences=conv(q), states=conv(x),
                             grad_controls=conv(gu), grad_states=conv(gx), inputs=I, **_plant_kw(plant, dist, conv))
    return [out[k] for k in s.ROLLOUT_GRAD_NAMES + s.PLANT_GRAD_NAMES]


def _plant_forward_data(n):
    I, H, S = NEWTON
    rng = np.random.default_rng(24)
    tan = td.soa_tangents(td.random_tangents(I, H, S, n, 25, K=1), n)
    tan.update(Ap=rng.standard_normal((1, 4, n)), Bp=rng.standard_normal((1, 2 * I, n)),
               Cp=rng.standard_normal((1, 2, n)), disturbance=rng.standard_normal((1, 2 * S, n)))
    return _plant_recorded(n) + (tan,)


def _plant_forward_run(s, d, conv):
    I, H, S = NEWTON
    ins, nl, plant, dist, q, x, tan = d
    return list(s.rollout_forward(S, *[conv(a) for a in ins], conv(nl), sequences=conv(q), states=conv(x),
                                  tangents={k: conv(v) for k, v in tan.items()}, inputs=I,
                                  plant=tuple(conv(a) for a in plant)))


_nonzero = lambda out: any(a[..., -1].any() for a in out)
_carried = lambda out: out[5][-1] == NEWTON[2] and np.all(out[3][:, -1] >= 0)       # the Newton loops: to the last step
_rows_live = lambda out: out[3][:, -1].any()                                        # PER_INSTANCE[3]: params_rows
# name -> (horizon of the handle, data, run, live)
LAUNCHERS = {
    "polish": (4, _polish_data, _polish_run, lambda out: out[1][-1] >= 0),
    "backward": (2, _backward_data, _backward_run, _nonzero),
    "forward": (2, _forward_data, _forward_run, lambda out: out[0][-1, :, -1].any()),
    "forward_k1": (2, lambda n: _forward_data(n, K=1), _forward_run, lambda out: out[0][-1, :, -1].any()),
    "exact_reg": (4, lambda n: compact_inputs(4, n), _exact_run, lambda out: out[3][-1] >= 0),
    "exact_ws": (7, lambda n: compact_inputs(7, n), _exact_run, lambda out: out[3][-1] >= 0),
    "exact_rows_reg": (4, lambda n: (*compact_inputs(4, n), cr.recipe_rows("all", 4, n)), _exact_run,
                       lambda out: out[3][-1] >= 0),
    "exact_rows_ws": (7, lambda n: (*compact_inputs(7, n), cr.recipe_rows("all", 7, n)), _exact_run,
                      lambda out: out[3][-1] >= 0),
    "compact_backward_reg": (4, lambda n: compact_grad_gpu._case(4, n), _compact_backward_run, _rows_live),
    "compact_backward_ws": (7, lambda n: compact_grad_gpu._case(7, n), _compact_backward_run, _rows_live),
    "compact_rows_backward_reg": (4, lambda n: compact_rows_gpu._case(4, n), _compact_backward_run, _rows_live),
    "compact_rows_backward_ws": (7, lambda n: compact_rows_gpu._case(7, n), _compact_backward_run, _rows_live),
    "newton": (NEWTON[1], _newton_data, _newton_run, _carried),
    "rollout_backward": (NEWTON[1], _rollout_backward_data, _rollout_backward_run, _nonzero),
    "rollout_forward": (NEWTON[1], _rollout_forward_data, _rollout_forward_run, _nonzero),
    "plant_newton": (NEWTON[1], _plant_newton_data, _plant_newton_run, _carried),
    "plant_backward": (NEWTON[1], _plant_backward_data, _plant_backward_run, _nonzero),
    "plant_forward": (NEWTON[1], _plant_forward_data, _plant_forward_run, _nonzero),
}
# (launcher, n): n = lanes, but for the single solve's tangent kernel with K = 3 directions, lanes = 3 n.  Of the three
# counts only 65280 divides by 3, so the thresholds are taken from both sides: 10880 instances (32640 lanes, the last
# grid of 64-lane blocks), 10881 (32643, the first of 128-lane blocks: three live lanes in the last block), 21760
# (65280) and 21761 (65283, the first of 256-lane blocks: three live lanes in the last block, and the boundaries
# between directions fall inside blocks).  The exact counts run with one direction (forward_k1).
CASES = [(name, n) for name in LAUNCHERS if name != "forward" for n in LANES] + \
    [("forward", n) for n in (10880, 10881, 21760, 21761)]


@functools.lru_cache(maxsize=None)
def _data(name, n):
    return LAUNCHERS[name][1](n)


@functools.lru_cache(maxsize=None)
def _host(name, n):
    """the host-only handle's outputs (never modified) and flags"""
    H, _, run, _ = LAUNCHERS[name]
    with MpcSolver(horizon=H, device=None) as s:
        out = run(s, _data(name, n), lambda a: a)
        return [_np(a) for a in out], s.last_flags


@pytest.mark.parametrize("name,n", CASES)
def test_device_equals_host_only_handle_bits_at_the_block_thresholds(name, n):
    H, _, run, live = LAUNCHERS[name]
    want, wflags = _host(name, n)
    with MpcSolver(horizon=H, device=0) as s:
        got = run(s, _data(name, n), _up)
        torch.cuda.synchronize()
        got, flags = [_np(a) for a in got], s.last_flags
    assert len(got) == len(want) and flags == wflags
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and a.shape[-1] == n, (name, i, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (name, i)
    assert live(got), "the last instance's column is trivial: its lane shows no work"


# ---- the fused polished step kernels: no host path, held to the loop composed from the public entries

FUSED = (2, 4, 2)       # I, H, S: polish_gpu's fused-against-composed test runs them at 130 lanes
POLISHED_FIELDS = polish_gpu.FIELDS
PLANT_FIELDS = ("controls", "states", "sequences", "iters", "status", "controls_inout", "v_inout")


def _fused_polished(s, ins, nl, n):
    """(composed, fused, status, residual_out) of rollout_polish_step_kernel's loop, DEVICE memory"""
    I, H, S = FUSED
    want = polish_gpu._composed(s, I, H, S, ins, nl, True, polish_gpu.TOL, polish_gpu.ROUNDS)
    got, _ = polish_gpu._fused(s, I, H, S, ins, nl, True, polish_gpu.TOL, polish_gpu.ROUNDS)
    return dict(zip(POLISHED_FIELDS, want)), dict(zip(POLISHED_FIELDS, got)), got[3], got[5]


def _fused_plant_polished(s, ins, nl, n):
    """the same of rollout_plant_polish_step_kernel's loop: the composed loop stages HOST arrays as plant_gpu's test
    does, the fused loop runs in DEVICE memory"""
    I, H, S = FUSED
    plant, dist = make_plant(ins, I, S)
    want = plant_gpu._composed(s, I, H, S, ins, nl, plant, dist, polished=True)
    c, v, ri, ro = (_up(np.zeros((r, n))) for r in (H * I, H * I, S, S))
    u, x, q, st, it = s.rollout_polished(S, *[_up(a) for a in ins], _up(nl), controls=c, v_state=v, inputs=I,
                                         tol=plant_gpu.TOL, max_rounds=plant_gpu.ROUNDS, want_iters=True,
                                         residuals=(ri, ro), **_plant_kw(plant, dist, _up))
    torch.cuda.synchronize()
    got = [_np(a) for a in (u, x, q, it, st, c, v)]
    return dict(zip(PLANT_FIELDS, want)), dict(zip(PLANT_FIELDS, got)), got[4], _np(ro)


@pytest.mark.parametrize("n", LANES)
@pytest.mark.parametrize("loop", [_fused_polished, _fused_plant_polished], ids=["polished", "plant_polished"])
def test_fused_polished_loops_equal_the_composed_loops_at_the_block_thresholds(loop, n):
    """The composed loop is the reference: its pieces are held to independent ones at these lane counts or in every
    family (the LANE solve to the oracle, polish_kernel to the host-only handle by the `polish` launcher above, the
    plant line is numpy)."""
    I, H, S = FUSED
    ins, nl, _, _ = polish_gpu._case(I, H, S, n, seed=H + I)
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        want, got, st, ro = loop(s, ins, nl, n)
    for name in want:
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == b.dtype and a.shape[-1] == n, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), name
    assert (st >= 0).any() and np.all(ro[st >= 0] <= polish_gpu.TOL), "no (instance, step) pair is polished"
    assert got["sequences"][:, -1].any(), "the last instance's column is trivial: its lane shows no work"
