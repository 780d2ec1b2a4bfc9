"""GPU tests of the warm-started exact compact solve (tpc_mpc_solve_batch_compact_exact_from,
MpcSolver.solve_batch_compact_exact(start=...), mpc_compact_exact(warm=...)): the device against the host-only handle
bit for bit through the register kernels (H = 4, 5) and the workspace kernels, shared and per-instance parameters, HOST
and DEVICE memory, with instances that have no start and invalid columns among them, in place; the fallback against
solve_batch_general + polish_batch_general on exactly the gathered instances; a five-step chain of a fitting loop; the
launcher's block thresholds; the handle's other entries untouched by a warm call; the autograd function against the
raw entries."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import compact_grad_common as cg
from tests.model import compact_rows_common as cr
from tests.model import compact_warm_common as cw
from tests.model.compact_exact_common import NAMES, ROUNDS, TOL, bits
from trajectory_controller_amd import CompactWarmStart, MpcSolver, capi, mpc_compact_exact
from trajectory_controller_amd.synth import compact_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("v", "delta_y", "delta_phi", "params", "params_rows", "kkt_residual")
NS = (1, 63, 65, 300, 4096)   # a lone lane, a partial wavefront, one lane into the second, a partial block, many blocks
SPOILED = (2, 9, 17, 25, 33, 41, 50)          # where the seven cases of cr.INVALID sit from 63 instances on (rows)
FWD = ("front", "rear", "sequence", "status", "fell_back", "residual_in", "residual_out")
MOVE = 0.01
KINDS = {"shared": ("shared", "default"), "rows": ("rows", "all")}


def _up(a, device=True):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if device else np.ascontiguousarray(a)


def _np(a):
    return None if a is None else np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)


def _solve(s, m, v, dy, dphi, start, device, fallback="none", rounds=ROUNDS):
    md = dict(over=m["over"], rows=_up(m["rows"], device))
    out = cw.solve(s, md, _up(v, device), _up(dy, device), _up(dphi, device), start=_up(start, device), rounds=rounds,
                   fallback=fallback)
    if device:
        torch.cuda.synchronize()
    return [_np(a) for a in out], s.last_flags


def _same_forward(got, want, cols=None, skip=()):
    for name, a, b in zip(FWD, got, want):
        if name in skip or a is None or b is None:
            continue
        if cols is not None:
            a, b = np.ascontiguousarray(a[..., cols]), np.ascontiguousarray(b[..., cols])
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert a.tobytes() == b.tobytes(), name


@functools.lru_cache(maxsize=None)
def _case(kind, H, n, seed=0):
    """a model one optimiser step after the one its starts come from, the mixed start of compact_warm_common (a quarter
    without a start), from 63 instances on the invalid columns of cr.INVALID (rows), and the host-only handle's answer;
    shared by the tests (never modified)"""
    v, dy, dphi = (a.copy() for a in compact_inputs(H, n))
    k, name = KINDS[kind]
    m = cw.model(k, name, H, n, MOVE)
    invalid = np.zeros(n, dtype=bool)
    with MpcSolver(horizon=H, device=None) as s:
        previous = cw.solve(s, cw.model(k, name, H, n), v, dy, dphi)[2]
        start = cw.mixed_start(previous, H, 3 + H + seed) if n > 1 else previous
        if kind == "rows" and n >= 63:
            m["rows"], v = cr.spoil(m["rows"], v, SPOILED)
            invalid[list(SPOILED[:6])] = True
        want, flags = _solve(s, m, v, dy, dphi, start, False)
    return dict(v=v, dy=dy, dphi=dphi, m=m, start=start, invalid=invalid, want=want, flags=flags)


# ---- 1. device against host: H = 4, 5 the register kernels, the others the workspace kernels

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("H", [1, 4, 5, 7, 10, 20, 40, 64])
def test_device_equals_host_only_handle_bits(H, kind, device):
    bad_flags = capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL
    with MpcSolver(horizon=H, device=0) as s:
        for n in NS:
            c = _case(kind, H, n)
            got, flags = _solve(s, c["m"], c["v"], c["dy"], c["dphi"], c["start"], device)
            _same_forward(got, c["want"])
            assert flags == c["flags"], n
            # the invalid columns raise theirs, the instances without a start none
            assert (flags & bad_flags) == (bad_flags if c["invalid"].any() else 0), n
            assert np.all(got[3][c["invalid"]] == -1) and not bits(got[2][:, c["invalid"]]).any()
            assert n == 1 or not np.isfinite(c["start"]).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("H", [4, 5, 7, 20])
def test_sequence_out_may_be_the_start(H, kind, device):
    n = 300
    c = _case(kind, H, n)
    lib = capi.load_library()
    with MpcSolver(horizon=H, device=0) as s:
        p = s._params(**c["m"]["over"])
        v, dy, dphi = (_up(c[k], device) for k in ("v", "dy", "dphi"))
        rows, start = _up(c["m"]["rows"], device), _up(c["start"].copy(), device)
        kw = {}
        if device:
            kw = dict(mem=capi.DEVICE, ptr=lambda t: t.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream,
                      new=lambda dtype, r=None: torch.empty(n if r is None else (r, n), device=DEV,
                                                            dtype=torch.float64 if dtype is np.float64 else torch.int32))
        rc, flags, front, rear, seq, st, rin, rout = cw.raw_from(lib, s._h, p, v, dy, dphi, start, rows=rows,
                                                                 in_place=True, **kw)
        if device:
            torch.cuda.synchronize()
    assert rc == 0 and flags == c["flags"] and seq is start
    _same_forward([_np(a) for a in (front, rear, seq, st, None, rin, rout)], c["want"])


# ---- 2. the fallback

def _reference(s, H, c, idx, rounds):
    """solve_batch_general (cold, zeroed controls) + polish_batch_general on exactly the instances idx of the case,
    expanded: the entry's outputs in FWD's order and the two calls' flags"""
    m = c["m"]
    sub = dict(over=m["over"], rows=None if m["rows"] is None else np.ascontiguousarray(m["rows"][:, idx]))
    th = cw.expanded(s, sub, H, c["v"][idx], c["dy"][idx], c["dphi"][idx])
    ins = [_up(th[k]) for k in NAMES]
    u = _up(np.zeros((2 * H, idx.size)))
    u0 = s.solve_batch_general(*ins, controls=u, inputs=2, **m["over"])
    f1 = s.last_flags
    _, st, rin, rout = s.polish_batch_general(*ins, u, tol=TOL, max_rounds=rounds, inputs=2)
    f2 = s.last_flags
    torch.cuda.synchronize()
    u, u0 = _np(u), _np(u0)
    assert np.array_equal(bits(u0[:, _np(st) < 0]), bits(u[:2, _np(st) < 0]))
    return [u[0], u[1], u, _np(st), None, _np(rin), _np(rout)], f1 | f2


def _check_fallback(kind, H, n, rounds):
    c = _case(kind, H, n, seed=rounds)
    invalid = c["invalid"]
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        none, nflags = _solve(s, c["m"], c["v"], c["dy"], c["dphi"], c["start"], True, "none", rounds)
        got, flags = _solve(s, c["m"], c["v"], c["dy"], c["dphi"], c["start"], True, "solve", rounds)
        fell = got[4]
        assert set(np.unique(fell)) <= {0, 1}
        assert np.array_equal(fell == 1, (none[3] == -1) & ~invalid)
        idx = np.flatnonzero(fell == 1)
        print(f"{kind} H={H} n={n} rounds={rounds}: fell back {idx.size}, left at -1 by its polish "
              f"{int((got[3][idx] < 0).sum())}, flags {flags:#x}")
        _same_forward(got, none, cols=np.flatnonzero(fell == 0), skip=("fell_back",))
        expect = nflags & ~capi.FLAG_NOT_POLISHED
        if idx.size:
            want, wflags = _reference(s, H, c, idx, rounds)
            _same_forward([a if a is None else a[..., idx] for a in got], want)
            expect |= wflags
        assert flags == expect
    return got, invalid


@pytest.mark.parametrize("kind,H", [("rows", 5), ("shared", 10), ("rows", 20)])
def test_fallback_is_solve_and_polish_on_the_gathered_instances(kind, H):
    got, invalid = _check_fallback(kind, H, 4096, ROUNDS)
    assert got[4].sum() > 0
    assert np.all(got[3][invalid] == -1) and not got[4][invalid].any()


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
@pytest.mark.parametrize("kind,H", [("shared", 5), ("rows", 10), ("shared", 20)])
def test_everybody_falls_back_without_rounds(kind, H, n):
    """max_rounds = 0 verifies only an instance whose clamped start already meets tol, which one optimiser step away
    from the start's own model none does"""
    got, invalid = _check_fallback(kind, H, n, 0)
    assert np.array_equal(got[4] == 1, ~invalid)


# ---- 3. a fitting loop's chain

@pytest.mark.parametrize("H", [20, 40])
def test_five_step_chain_falls_back_no_more_than_the_cold_entry(H):
    n = 4096
    v, dy, dphi = compact_inputs(H, n)
    tv, ty, tp = _up(v), _up(dy), _up(dphi)
    kw = dict(tol=TOL, max_rounds=ROUNDS, fallback="solve", want_sequence=True)
    counts = []
    with MpcSolver(horizon=H, device=0) as s:
        seq = None
        for step in range(5):
            over = cw.model("shared", "default", H, n, MOVE, steps=step)["over"]
            _, _, _, cst, cfell = s.solve_batch_compact_exact(tv, ty, tp, **kw, **over)
            _, _, seq, wst, wfell = s.solve_batch_compact_exact(tv, ty, tp, start=seq, **kw, **over)
            torch.cuda.synchronize()
            counts.append((int(cfell.sum()), int(wfell.sum()), float(cst[cst >= 0].double().mean()),
                           float(wst[(wst >= 0) & (wfell == 0)].double().mean())))
    for step, (cold, warm, crounds, wrounds) in enumerate(counts):
        print(f"H={H} step {step + 1}: fell back cold {cold}, warm {warm}; mean rounds (status >= 0) cold {crounds:.2f}, "
              f"warm phase 1 {wrounds:.2f}")
    assert counts[0][0] == counts[0][1]                  # the first step has no start: the cold call
    for cold, warm, _, _ in counts[1:]:
        assert warm <= cold


# ---- 4. the launcher at the block thresholds of rollout_grad_block

@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [32641, 65280, 65281])
@pytest.mark.parametrize("H", [4, 7])
def test_launch_shapes(H, n, kind):
    v, dy, dphi = compact_inputs(H, n)
    k, name = KINDS[kind]
    m = cw.model(k, name, H, n, MOVE)
    start = cw.mixed_start(cw.random_start(H, n, 9) * 0.1, H, 10)
    with MpcSolver(horizon=H, device=None) as s:
        want, wflags = _solve(s, m, v, dy, dphi, start, False)
    with MpcSolver(horizon=H, device=0) as s:
        got, flags = _solve(s, m, v, dy, dphi, start, True)
    _same_forward(got, want)
    assert flags == wflags
    assert (got[3] >= 0).sum() >= 0.8 * n


# ---- 5. the handle's other entries: the working sets are shared

@pytest.mark.parametrize("kind", list(KINDS))
def test_other_entries_return_the_same_bytes_around_a_warm_call(kind):
    H, n = 10, 300
    c = _case(kind, H, n)
    tv, ty, tp = (_up(a) for a in compact_inputs(H, n))
    rows = _up(cr.recipe_rows("all", H, n))
    gf, gr, gs = (_up(a) for a in cg.grad_in(H, n, 17 + H, sequence=True))

    def others(s):
        out = list(s.solve_batch_compact_exact(tv, ty, tp, tol=TOL, max_rounds=ROUNDS, want_sequence=True,
                                               want_residuals=True))
        out += list(s.solve_batch_compact_exact_backward(tv, ty, tp, out[2], gf, gr, gs, status=out[3],
                                                         want=ALL).values())
        fwd = s.solve_batch_compact_exact(tv, ty, tp, tol=TOL, max_rounds=ROUNDS, want_sequence=True, params_rows=rows)
        out += list(fwd)
        out += list(s.solve_batch_compact_exact_backward(tv, ty, tp, fwd[2], gf, gr, gs, status=fwd[3], want=ALL,
                                                         params_rows=rows).values())
        torch.cuda.synchronize()
        return [_np(a).tobytes() for a in out if a is not None]

    with MpcSolver(horizon=H, device=0) as s:
        before = others(s)
        got, _ = _solve(s, c["m"], c["v"], c["dy"], c["dphi"], c["start"], True, "solve")
        assert others(s) == before
        again, _ = _solve(s, c["m"], c["v"], c["dy"], c["dphi"], c["start"], True, "solve")
        _same_forward(again, got)


# ---- 6. autograd

@pytest.mark.parametrize("per_instance", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("H", [4, 20])
def test_autograd_carries_the_sequence_from_call_to_call(H, per_instance):
    n = 300
    v, dy, dphi = compact_inputs(H, n)
    rng = np.random.default_rng(4)
    cf, cb = _up(rng.standard_normal(n)), _up(rng.standard_normal(n))
    if per_instance:
        w1 = cr.recipe_rows("weights", H, n)[cr.W]
    else:
        w1 = np.array([20.0, 7.0, 0.0005, 10.0])
    w2 = w1 * (1.0 + MOVE * cw.SIGNS).reshape((4,) + (1,) * (w1.ndim - 1))
    with MpcSolver(horizon=H, device=0) as s:

        def raw(w, start):
            if per_instance:
                rows = cr.shared_rows(s.params, n)
                rows[cr.W] = w
                kw = dict(params_rows=_up(rows))
            else:
                kw = dict(zip(cw.WEIGHTS, w.tolist()))
            out = s.solve_batch_compact_exact(tv.detach(), ty.detach(), tp.detach(), tol=TOL, max_rounds=ROUNDS,
                                              want_sequence=True, start=start, **kw)
            return out, kw

        warm = CompactWarmStart()
        seqs = []
        for w, start_is in ((w1, None), (w2, 0)):
            tv, ty, tp = (_up(a).requires_grad_() for a in (v, dy, dphi))
            weights = (_up(w) if per_instance else torch.from_numpy(w.copy())).requires_grad_()
            front, rear = mpc_compact_exact(s, tv, ty, tp, weights=weights, tol=TOL, max_rounds=ROUNDS, warm=warm)
            seqs.append(warm.sequence)
            assert not warm.sequence.requires_grad and tuple(warm.sequence.shape) == (2 * H, n)
            # the first call is the cold entry, the second the raw entry from the first call's sequence
            (rf, rr, seq, st, _), kw = raw(w, None if start_is is None else seqs[start_is])
            torch.cuda.synchronize()
            assert _np(front.detach()).tobytes() == _np(rf).tobytes()
            assert _np(rear.detach()).tobytes() == _np(rr).tobytes()
            assert _np(warm.sequence).tobytes() == _np(seq).tobytes()
            (cf * front + cb * rear).sum().backward()
            back = s.solve_batch_compact_exact_backward(tv.detach(), ty.detach(), tp.detach(), seq, cf, cb, status=st,
                                                        want=ALL if per_instance else ALL[:4] + ALL[5:], **kw)
            torch.cuda.synchronize()
            for t, k in ((tv, "v"), (ty, "delta_y"), (tp, "delta_phi")):
                assert _np(t.grad).tobytes() == _np(back[k]).tobytes(), k
            if per_instance:
                assert _np(weights.grad).tobytes() == _np(back["params_rows"][cr.W]).tobytes()
            else:
                assert _np(weights.grad).tobytes() == _np(back["params"][cr.W]).tobytes()
        assert seqs[0] is not seqs[1] and _np(seqs[0]).tobytes() != _np(seqs[1]).tobytes()
        # a changed n is a cold call, and the holder follows it
        m = 65
        front, _ = mpc_compact_exact(s, _up(v[:m]), _up(dy[:m]), _up(dphi[:m]), tol=TOL, max_rounds=ROUNDS, warm=warm)
        want = s.solve_batch_compact_exact(_up(v[:m]), _up(dy[:m]), _up(dphi[:m]), tol=TOL, max_rounds=ROUNDS)[0]
        torch.cuda.synchronize()
        assert _np(front).tobytes() == _np(want).tobytes() and tuple(warm.sequence.shape) == (2 * H, m)
