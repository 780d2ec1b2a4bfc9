"""GPU tests of the launch shapes of the one-lane-per-instance fp64 kernels.  rollout_grad_block() gives blocks of 64
lanes below 32641 lanes, of 128 from 32641 and of 256 from 65281, and every launcher of the family uses it (the tangent
kernels with lanes = K * n).  Here each launcher runs at 32641 lanes (the first grid of 128-lane blocks, one live lane
in the last block), 65280 (the last one, every block full) and 65281 (the first grid of 256-lane blocks, one live lane
in the last block), DEVICE memory, with the smallest problem that still runs every loop, and must return the host-only
handle's bits; the last instance's column must show that its lane did work.  (With K = 3 directions the lane count is
3 n, which meets only 65280 exactly: see CASES.)

rollout_polished and the plant entries take the same block choice through the same function but have no host path to
compare with, so they are left out."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.bindings import Oracle
from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.model import mpc_rollout_tangent_dense as td
from tests.model.compact_exact_common import ROUNDS as EXACT_ROUNDS, TOL
from tests.test_rollout_newton_host import soa_inputs
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
    out = s.solve_batch_compact_exact(*[conv(a) for a in d], tol=TOL, max_rounds=EXACT_ROUNDS, fallback="none",
                                      want_sequence=True, want_residuals=True)
    assert out[4] is None       # fell_back: not with fallback="none"
    return [a for a in out if a is not None]


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


_nonzero = lambda out: any(a[..., -1].any() for a in out)
# name -> (horizon of the handle, data, run, live)
LAUNCHERS = {
    "polish": (4, _polish_data, _polish_run, lambda out: out[1][-1] >= 0),
    "backward": (2, _backward_data, _backward_run, _nonzero),
    "forward": (2, _forward_data, _forward_run, lambda out: out[0][-1, :, -1].any()),
    "forward_k1": (2, lambda n: _forward_data(n, K=1), _forward_run, lambda out: out[0][-1, :, -1].any()),
    "exact_reg": (4, lambda n: compact_inputs(4, n), _exact_run, lambda out: out[3][-1] >= 0),
    "exact_ws": (7, lambda n: compact_inputs(7, n), _exact_run, lambda out: out[3][-1] >= 0),
    "newton": (NEWTON[1], _newton_data, _newton_run,
               lambda out: out[5][-1] == NEWTON[2] and np.all(out[3][:, -1] >= 0)),
    "rollout_backward": (NEWTON[1], _rollout_backward_data, _rollout_backward_run, _nonzero),
    "rollout_forward": (NEWTON[1], _rollout_forward_data, _rollout_forward_run, _nonzero),
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
