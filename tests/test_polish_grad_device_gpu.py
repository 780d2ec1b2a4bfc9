"""GPU tests of the device-only side of tpc_mpc_polish_batch_general and tpc_mpc_solve_batch_general_backward: what the
host-only handle cannot show, because it runs the arithmetic on the calling thread straight on the caller's arrays.
On a device handle, through the C entries, in HOST (staged) and DEVICE memory: the smallest shapes, a shard of a wider
batch (ld > n, so the workspace stride n and the array stride ld differ), every pattern of NULL outputs, and flagged
instances raised from two wavefronts beside clean lanes.  Every comparison is bit equality with the host-only handle.

Inputs: tests/model/mpc_grad_dense.mixed_batch (active bounds, a pinned input, zero state weights); the polish starts
from the oracle's controls at eps 0.01 (tests/test_polish_host.py), the backward is taken at clipped noise with N(0, 1)
grad_controls (as tests/test_grad_gpu.py)."""
import functools
import itertools
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import mpc_grad_dense as dense
from tests.test_grad_host import _call, _rows
from tests.test_polish_host import _raw, _wide
from trajectory_controller_amd import MpcSolver, capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = dense.NAMES
SENTINEL = 12345.0
SMALL = [(1, 1), (2, 1), (1, 2), (2, 3), (2, 7)]
MEM = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
POLISH_OUTS = ("u0", "status", "residual_in", "residual_out")
BAD = [0, 63, 64, 69]      # flagged columns: both wavefronts of a batch of 70, first and last lanes


class _Buf:
    """An array [rows, ld] in HOST or DEVICE memory the way _raw and _call take one: .ctypes.data is the address of
    column k0"""

    def __init__(self, a, device, k0=0):
        a = np.array(a, order="C", copy=True)
        assert a.ndim == 2
        self.a = torch.from_numpy(a).to(DEV) if device else a
        base = self.a.data_ptr() if device else self.a.ctypes.data
        self.ctypes = types.SimpleNamespace(data=base + k0 * a.itemsize)

    def numpy(self):
        return self.a.cpu().numpy() if torch.is_tensor(self.a) else self.a


def _embed(a, ld, k0, pad):
    """the columns of a at k0 .. of an array of ld columns filled with pad"""
    w = np.full((a.shape[0], ld), pad, dtype=a.dtype)
    w[:, k0:k0 + a.shape[1]] = a
    return w


def _polish(s, I, H, ins, u, device, present=POLISH_OUTS, ld=None, k0=0):
    """tpc_mpc_polish_batch_general on the n columns ins / u hold, embedded at k0 in arrays of ld columns (inputs padded
    with NaN, in/outs and outputs with sentinels): (rc, flags, {name: the whole array})"""
    n = u.shape[1]
    ld = n if ld is None else ld
    bufs = {k: _Buf(_embed(ins[k], ld, k0, np.nan), device, k0) for k in NAMES}
    out = dict(controls=_Buf(_embed(u, ld, k0, SENTINEL), device, k0))
    rows = dict(u0=I, status=1, residual_in=1, residual_out=1)
    for k in present:
        fill = np.full((rows[k], ld), -7, dtype=np.int32) if k == "status" else np.full((rows[k], ld), SENTINEL)
        out[k] = _Buf(fill, device, k0)
    rc, flags = _raw(s._h, H, I, n, ld, bufs, out["controls"], status=out.get("status"), rin=out.get("residual_in"),
                     rout=out.get("residual_out"), u0=out.get("u0"), mem=capi.DEVICE if device else capi.HOST)
    if device:
        torch.cuda.synchronize()
    return rc, flags, {k: b.numpy() for k, b in out.items()}


def _backward(s, I, H, ins, u, g, device, present=None, ld=None, k0=0):
    """tpc_mpc_solve_batch_general_backward the same way: (rc, flags, {name: the whole array})"""
    n = u.shape[1]
    ld = n if ld is None else ld
    rows = _rows(I, H)
    present = tuple(rows) if present is None else present
    bufs = {k: _Buf(_embed(ins[k], ld, k0, np.nan), device, k0) for k in NAMES}
    bu, bg = (_Buf(_embed(a, ld, k0, np.nan), device, k0) for a in (u, g))
    out = {k: _Buf(np.full((rows[k], ld), SENTINEL), device, k0) for k in present}
    rc, flags = _call(s._h, H, I, n, ld, bufs, bu, bg, out, mem=capi.DEVICE if device else capi.HOST)
    if device:
        torch.cuda.synchronize()
    return rc, flags, {k: b.numpy() for k, b in out.items()}


def _polish_inputs(I, H, n):
    """fresh copies of ({name: [rows, n]}, controls [H*I, n]): mixed_batch and the oracle's controls at eps 0.01"""
    return _wide(I, H, n, n)


@functools.lru_cache(maxsize=None)
def _grad_batch(I, H, n):
    th = dense.mixed_batch(I, H, n)
    ins = {k: dense.soa(th[k], n) for k in NAMES}
    rng = np.random.default_rng(1 + 17 * H + I)
    u = np.clip(rng.standard_normal((H * I, n)) * 0.3, np.tile(ins["lo"], (H, 1)), np.tile(ins["hi"], (H, 1)))
    return ins, np.ascontiguousarray(u), rng.standard_normal((H * I, n))


def _grad_inputs(I, H, n):
    """fresh copies of ({name: [rows, n]}, controls, grad_controls): mixed_batch, clipped noise, N(0, 1)"""
    ins, u, g = _grad_batch(I, H, n)
    return {k: a.copy() for k, a in ins.items()}, u.copy(), g.copy()


@functools.lru_cache(maxsize=None)
def _polish_host(I, H, n):
    ins, u = _polish_inputs(I, H, n)
    with MpcSolver(horizon=H, device=None) as s:
        return _polish(s, I, H, ins, u, False)


@functools.lru_cache(maxsize=None)
def _backward_host(I, H, n):
    with MpcSolver(horizon=H, device=None) as s:
        return _backward(s, I, H, *_grad_inputs(I, H, n), False)


def _same(got, want, cols=None, names=None):
    for k in (got if names is None else names):
        a, b = got[k], want[k]
        if cols is not None:
            a, b = np.ascontiguousarray(a[:, cols]), np.ascontiguousarray(b[:, cols])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), k


# ---- 1. small shapes: one lane, one wavefront less one, exactly one, one more, and five wavefronts less 63 ------------

@MEM
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("I,H", SMALL)
def test_polish_small_shapes(I, H, n, device):
    rc0, wflags, want = _polish_host(I, H, n)
    ins, u = _polish_inputs(I, H, n)
    with MpcSolver(horizon=H, device=0) as s:
        rc, flags, got = _polish(s, I, H, ins, u, device)
    assert rc0 == rc == 0 and flags == wflags
    assert set(got) == {"controls"} | set(POLISH_OUTS)
    _same(got, want)


@MEM
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("I,H", SMALL)
def test_backward_small_shapes(I, H, n, device):
    rc0, wflags, want = _backward_host(I, H, n)
    with MpcSolver(horizon=H, device=0) as s:
        rc, flags, got = _backward(s, I, H, *_grad_inputs(I, H, n), device)
    assert rc0 == rc == 0 and flags == wflags == 0
    assert set(got) == set(_rows(I, H))
    _same(got, want)


# ---- 2. a shard of a wider batch: ld = 200 > n = 70, so the arrays' stride and the workspace's differ -----------------

LD, K0, M = 200, 37, 70


def _check_shard(got, want):
    """the shard's columns are the contiguous call's bits, every sentinel outside it is intact"""
    for k, a in got.items():
        assert np.ascontiguousarray(a[:, K0:K0 + M]).tobytes() == want[k].tobytes(), k
        pad = -7 if k == "status" else SENTINEL
        assert np.all(a[:, :K0] == pad) and np.all(a[:, K0 + M:] == pad), k


@MEM
@pytest.mark.parametrize("I,H", [(2, 7), (1, 3)])
def test_polish_shard_of_a_wider_batch(I, H, device):
    rc0, wflags, want = _polish_host(I, H, M)
    ins, u = _polish_inputs(I, H, M)
    with MpcSolver(horizon=H, device=0) as s:
        rc, flags, got = _polish(s, I, H, ins, u, device, ld=LD, k0=K0)
    # flags 0: nothing non-finite was seen, so no NaN of the padding was read
    assert rc0 == rc == 0 and flags == wflags == 0
    assert set(got) == {"controls"} | set(POLISH_OUTS)
    _check_shard(got, want)


@MEM
@pytest.mark.parametrize("I,H", [(2, 7), (1, 3)])
def test_backward_shard_of_a_wider_batch(I, H, device):
    rc0, wflags, want = _backward_host(I, H, M)
    with MpcSolver(horizon=H, device=0) as s:
        rc, flags, got = _backward(s, I, H, *_grad_inputs(I, H, M), device, ld=LD, k0=K0)
    assert rc0 == rc == 0 and flags == wflags == 0
    assert set(got) == set(_rows(I, H)) and len(got) == 10
    _check_shard(got, want)


# ---- 3. NULL outputs --------------------------------------------------------------------------------------------------

@MEM
def test_polish_null_outputs(device):
    I, H, n = 2, 7, 70
    _, wflags, want = _polish_host(I, H, n)
    with MpcSolver(horizon=H, device=0) as s:
        for r in range(len(POLISH_OUTS) + 1):
            for present in itertools.combinations(POLISH_OUTS, r):
                ins, u = _polish_inputs(I, H, n)
                rc, flags, got = _polish(s, I, H, ins, u, device, present=present)
                assert rc == 0 and flags == wflags, present
                assert set(got) == {"controls"} | set(present)
                _same(got, want)


@MEM
def test_backward_null_outputs(device):
    I, H, n = 2, 7, 70
    _, wflags, want = _backward_host(I, H, n)
    names = tuple(_rows(I, H))
    with MpcSolver(horizon=H, device=0) as s:
        for present in [names] + [(k,) for k in names] + [("dB", "dlower", "dtargets"), ()]:
            rc, flags, got = _backward(s, I, H, *_grad_inputs(I, H, n), device, present=present)
            assert rc == 0 and flags == wflags == 0, present
            assert set(got) == set(present)
            _same(got, want)


# ---- 4. flagged instances: raised by lanes of two wavefronts beside clean lanes, and the flag word reset ---------------

@MEM
@pytest.mark.parametrize("what,flag", [("targets", capi.FLAG_NONFINITE), ("controls", capi.FLAG_NONFINITE),
                                       ("x0", capi.FLAG_NONFINITE), ("R", capi.FLAG_BAD_MODEL),
                                       ("bounds", capi.FLAG_BAD_MODEL)])
def test_polish_flagged_instances_are_left_alone(what, flag, device):
    I, H, n = 2, 6, 70
    _, cflags, clean = _polish_host(I, H, n)
    ins, u = _polish_inputs(I, H, n)
    if what == "targets":
        ins["targets"][3, BAD] = np.nan
    elif what == "controls":
        u[H * I - 1, BAD] = np.inf
    elif what == "x0":
        ins["x0"][1, BAD] = -np.inf
    elif what == "R":
        ins["R"][1, BAD] = 0.0
    else:
        ins["hi"][0, BAD] = ins["lo"][0, BAD] - 0.1
    with MpcSolver(horizon=H, device=None) as hs:
        _, wflags, want = _polish(hs, I, H, ins, u, False)
    with MpcSolver(horizon=H, device=0) as s:
        rc, flags, got = _polish(s, I, H, ins, u, device)
        rc2, flags2, again = _polish(s, I, H, *_polish_inputs(I, H, n), device)      # the flag word is reset
    assert rc == 0 and flags == wflags == flag | cflags and flags & flag
    _same(got, want)
    # the flagged columns are left alone with status -1, every other column is the clean run's
    assert np.all(got["status"][0, BAD] == -1)
    assert got["controls"][:, BAD].tobytes() == u[:, BAD].tobytes()
    assert got["u0"][:, BAD].tobytes() == u[:I, BAD].tobytes()
    _same(got, clean, cols=np.setdiff1d(np.arange(n), BAD), names=("controls", "u0", "status"))
    assert rc2 == 0 and flags2 == cflags == 0
    _same(again, clean)


@MEM
@pytest.mark.parametrize("what,flag", [("targets", capi.FLAG_NONFINITE), ("grad", capi.FLAG_NONFINITE),
                                       ("controls", capi.FLAG_NONFINITE), ("R", capi.FLAG_BAD_MODEL),
                                       ("bounds", capi.FLAG_BAD_MODEL)])
def test_backward_flags_zero_the_instance(what, flag, device):
    I, H, n = 2, 6, 70
    _, cflags, clean = _backward_host(I, H, n)
    ins, u, g = _grad_inputs(I, H, n)
    if what == "targets":
        ins["targets"][3, BAD] = np.nan
    elif what == "grad":
        g[H * I - 1, BAD] = np.inf
    elif what == "controls":
        u[0, BAD] = np.nan
    elif what == "R":
        ins["R"][1, BAD] = 0.0
    else:
        ins["hi"][0, BAD] = ins["lo"][0, BAD] - 0.1
    with MpcSolver(horizon=H, device=None) as hs:
        _, wflags, want = _backward(hs, I, H, ins, u, g, False)
    with MpcSolver(horizon=H, device=0) as s:
        rc, flags, got = _backward(s, I, H, ins, u, g, device)
        rc2, flags2, again = _backward(s, I, H, *_grad_inputs(I, H, n), device)      # the flag word is reset
    assert rc == 0 and flags == wflags == flag and cflags == 0
    _same(got, want)
    for k, a in got.items():
        assert np.all(a[:, BAD] == 0.0), k
    _same(got, clean, cols=np.setdiff1d(np.arange(n), BAD))
    assert rc2 == 0 and flags2 == 0
    _same(again, clean)
