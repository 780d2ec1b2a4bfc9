"""GPU tests of MpcSolver's argument rules for CUDA tensors, on the shapes and tables of tests/test_solver_args_host.py:
a tensor is never copied, so a non-contiguous one, a CPU one, one of another dtype and one of another shape are each a
ValueError before anything is launched, for the arrays an entry reads and for those it writes into; and every entry
launches on torch's current stream -- a call under a side stream gives the bits of the call on the default stream.
Nothing here launches what the suite does not launch at larger sizes elsewhere."""
import numpy as np
import pytest

from tests.model import follow_ref as fr
import types

from tests.test_solver_args_host import ENTRIES as HOST_ENTRIES, H, I, MODEL, N, arguments as host_arguments, base, model
from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd._arrays import Arrays, _raw_stream

pytestmark = pytest.mark.gpu

FP32_ENTRIES = ("solve_batch_general", "rollout")     # follow the solver's dtype: checked on an "f32" solver
# the sharded entries take tensors only; a handle without a communicator is a world of one: the shard is the batch
SHARDED = {
    "solve_batch_compact_sharded": (
        lambda s, a: s.solve_batch_compact_sharded(N, a["v"], a["dy"], a["dphi"], want_iters=True, want_flags=True),
        ("v", "dy", "dphi"), (), False),
    "solve_batch_general_sharded": (
        lambda s, a: s.solve_batch_general_sharded(*model(a), inputs=I, want_iters=True), MODEL, (), False),
}
ENTRIES = {**{k: e for k, e in HOST_ENTRIES.items() if not k.endswith("[plant]")}, **SHARDED}
NAMES = list(ENTRIES)


def arguments(name):
    return {k: base()[k] for k in ENTRIES[name][1]} if name in SHARDED else host_arguments(name)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def on_device(torch, a, f32=False):
    """the host tables' arguments as CUDA tensors (fresh ones: some are written)"""
    out = {}
    for k, x in a.items():
        t = torch.from_numpy(np.array(x, order="C")).cuda()
        out[k] = t.float() if f32 and t.dtype == torch.float64 else t
    return out


def bad_tensors(torch, t):
    if t.ndim == 1:
        strided = t.repeat_interleave(2)[::2]
    else:
        strided = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not strided.is_contiguous() and torch.equal(strided, t)
    other = {torch.float64: torch.float32, torch.float32: torch.float64, torch.int32: torch.int64}[t.dtype]
    shape = list(t.shape)
    shape[-2 if t.ndim > 1 else 0] += 1
    return (("non-contiguous", strided), ("cpu", t.cpu()), ("dtype", t.to(other)),
            ("shape", torch.zeros(shape, dtype=t.dtype, device=t.device)))


@pytest.mark.parametrize("name", NAMES)
def test_a_tensor_that_would_need_a_copy_is_a_value_error(torch_cuda, name):
    torch = torch_cuda
    call, reads, writes, _ = ENTRIES[name]
    f32 = name in FP32_ENTRIES
    with MpcSolver(horizon=H, device=0, dtype="f32" if f32 else "f64") as s:
        for key in reads + writes:
            a = on_device(torch, arguments(name), f32)
            good = on_device(torch, {key: base()[key]}, f32)[key]
            if key in ("rin", "rout"):
                a.update(on_device(torch, {k: base()[k] for k in ("rin", "rout")}))
            for label, bad in bad_tensors(torch, good):
                if name == "solve_batch_compact_exact" and key == "v" and label == "shape":
                    continue      # v's own length is n: the other two then disagree, which the next keys show
                with pytest.raises(ValueError):
                    call(s, {**a, key: bad})
                    pytest.fail(f"{name}: {key} {label} was accepted")


def test_compact_and_mixed_tensors(torch_cuda):
    torch = torch_cuda
    a = on_device(torch, {k: base()[k] for k in ("v", "dy", "dphi", "horizons")})
    v, dy, dphi, hz = a["v"], a["dy"], a["dphi"], a["horizons"]
    front, rear = torch.empty_like(v), torch.empty_like(v)
    with MpcSolver(horizon=H, device=0) as s:
        for i in range(3):
            for label, bad in bad_tensors(torch, (v, dy, dphi)[i]):
                if i == 0 and label == "shape":
                    continue
                args = [v, dy, dphi]
                args[i] = bad
                with pytest.raises(ValueError):
                    s.solve_batch_compact(*args)
                with pytest.raises(ValueError):
                    s.solve_batch_compact_mixed(hz, *args)
        for label, bad in bad_tensors(torch, front):
            with pytest.raises(ValueError):
                s.solve_batch_compact(v, dy, dphi, out=(bad, rear))
            with pytest.raises(ValueError):
                s.solve_batch_compact(v, dy, dphi, out=(front, bad))
        with pytest.raises(ValueError):
            s.solve_batch_compact_mixed(torch.full((N + 1,), H, dtype=torch.int32, device=v.device), v, dy, dphi)


def follow_arguments(torch):
    b = fr.random_batch(N, 6, 5)
    return [torch.from_numpy(np.array(b[k], order="C")).cuda() for k in fr.FIELDS]


@pytest.mark.parametrize("horizon_entry", [False, True])
def test_follow_tensors(torch_cuda, horizon_entry):
    torch = torch_cuda
    good = follow_arguments(torch)
    spacing = torch.full((N,), 0.05, dtype=torch.float32, device="cuda")
    with MpcSolver(horizon=H, device=0) as s:
        entry = s.follow_batch_horizon if horizon_entry else s.follow_batch
        for i in range(len(good)):
            for label, bad in bad_tensors(torch, good[i]):
                if i == 0 and label == "shape":
                    continue      # pos_x's own shape is [max_points, n]
                args = list(good)
                args[i] = bad
                with pytest.raises(ValueError):
                    entry(*args)
        if horizon_entry:
            for label, bad in bad_tensors(torch, spacing):
                with pytest.raises(ValueError):
                    entry(*good, step_spacing=bad)


def same_bits(torch, got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
                                         for g, w in zip(got, want))


def on_both_streams(torch, call):
    """the call's outputs on the default stream and under a side stream"""
    res = []
    side = torch.cuda.Stream()
    for stream in (None, side):
        if stream is None:
            out = call()
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                out = call()
        torch.cuda.synchronize()
        out = list(out.values()) if isinstance(out, dict) else list(out) if isinstance(out, tuple) else [out]
        res.append([x.cpu().numpy() for x in out if x is not None])
    return res


@pytest.mark.parametrize("name", NAMES)
def test_the_current_stream_is_the_calls_stream(torch_cuda, name):
    torch = torch_cuda
    with MpcSolver(horizon=H, device=0) as s:
        want, got = on_both_streams(torch, lambda: ENTRIES[name][0](s, on_device(torch, arguments(name))))
    assert want and same_bits(torch, got, want)


def test_the_current_stream_is_the_compact_and_follow_calls_stream(torch_cuda):
    torch = torch_cuda
    a = on_device(torch, {k: base()[k] for k in ("v", "dy", "dphi", "horizons")})
    follow = follow_arguments(torch)
    with MpcSolver(horizon=H, device=0) as s:
        for call in (lambda: s.solve_batch_compact(a["v"], a["dy"], a["dphi"], want_iters=True),
                     lambda: s.solve_batch_compact_mixed(a["horizons"], a["v"], a["dy"], a["dphi"], want_iters=True),
                     lambda: s.follow_batch(*follow, want_iters=True),
                     lambda: s.follow_batch_horizon(*follow, want_iters=True, want_targets=True)):
            want, got = on_both_streams(torch, call)
            assert want and same_bits(torch, got, want)


def test_the_stream_handed_to_the_library_is_torchs_current_one(torch_cuda):
    """what the bit comparisons above cannot see (they synchronise the device): the helper reads the stream that is
    current at the call, by either way of reading it, and _run hands exactly that to the entry"""
    torch = torch_cuda
    t = torch.zeros(N, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    seen = []

    def entry(handle, params, *args):
        seen.append(args)
        return capi.OK
    without_getter = types.SimpleNamespace(_C=types.SimpleNamespace(), cuda=torch.cuda)
    with MpcSolver(horizon=H, device=0) as s:
        for stream in (torch.cuda.default_stream(), side):
            with torch.cuda.stream(stream):
                ar = Arrays(t)
                assert (ar.stream.value or 0) == stream.cuda_stream == torch.cuda.current_stream().cuda_stream
                assert _raw_stream(torch, t) == _raw_stream(without_getter, t) == stream.cuda_stream
                s._run(entry, s.params, ar, 1, 2)
                assert seen[-1][:2] == (1, 2) and seen[-1][-2] == capi.DEVICE and seen[-1][-1] is ar.stream
                s._run(entry, s.params, ar, 3, want_flags=False, mem=False)
                assert seen[-1][0] == 3 and seen[-1][-2] is None and seen[-1][-1] is ar.stream


def test_a_numpy_call_returns_fresh_arrays_whatever_out_is(torch_cuda):
    a = base()
    with MpcSolver(horizon=H, device=0) as s:
        want = s.solve_batch_compact(a["v"], a["dy"], a["dphi"])
        mine = (np.full(N, 7.0), np.full(N, 7.0))
        for out in (mine, ([0.0] * N, None), (np.zeros(N, dtype=np.float32), np.zeros((N, 2)).T[0])):
            got = s.solve_batch_compact(a["v"], a["dy"], a["dphi"], out=out)
            assert all(isinstance(g, np.ndarray) and g is not o and g.tobytes() == w.tobytes()
                       for g, o, w in zip(got, out, want))
        assert np.all(mine[0] == 7.0) and np.all(mine[1] == 7.0)
