"""`-m gpu`: the refill protocol of the persistent kernels next to their references, on grids of 1 and 3 wavefronts.

Every fast family is a persistent grid whose lanes (or groups of lanes) pull the next instance from a sorted queue when
theirs finishes: per-lane state is overwritten while the neighbours keep iterating, momentum v is reset or taken from the
record (kMetaVInit), the queue has a dealt part read one pass ahead and a ticket part, a lane learns that the queue is
empty from `t >= n_queue`, passes wait for RefillBatch lanes, and a stop and a cap can fall in the same pass (mpc_ub.h,
mpc_group.h, mpc_groupg.h, and the hand-written N = 20 / N = 10 loops of mpc_ub_pg_asm*.h).  On the full chip the grid
holds 65 536 instances at once, so the bit-exact tests of the other modules -- a few thousand instances -- give every lane
at most one instance and never run a second pass.  Here the grid is pinned (tpc_mpc_x_set_group_share -> Workspace::
max_waves, which the LANE_FMA compact, asm, GROUP and GROUPG launchers clamp their grid to), so that a few hundred
instances put four to six through every lane, and the CPU references decide every bit:
  * LANE_FMA compact against the CPU model (tests/model): bits and iteration counts, tests/test_ub_gpu.py's statement;
  * GROUP compact and GROUPG general against the oracle: identical iteration counts, |du| <= 1e-9, bound-sitting controls
    bit for bit -- tests/test_group_gpu.py's and tests/test_groupg_gpu.py's statements and tolerances.

Sizes.  L = what the pinned grid holds at once (64 per wavefront, 64 / G for the group families).  n = L - 1, L, L + 1 (the
queue ends inside the first ticket), 4 L (the last ticket request lands exactly on n_queue), 4 L + 37 / + 5 (a ragged tail
below RefillBatch); N <= 10 on one wavefront also n = 300: per_wave = 285, five dealt passes with prefetch and a ticket part
of 15.  fp32 LANE_FMA at N = 10 / 20 has workgroups of two wavefronts: its grids are the smallest and the third-smallest the
launcher produces (one and three workgroups; the smallest is asked for as a share of ONE wavefront, which used to round down
to a grid of zero -- mpc_ub_inst.hip, pg_launch).

Every test shows that it exercised refills, as conditions on its inputs: at the 4 L sizes at least 2 L instances enter the
projected-gradient phase by the reference's own iteration counts (iters > smo_iters), and last_lane_stats() reports more
refill passes than the grid has wavefronts.

NOT covered: the LANE, LANEX and general-form LANE_FMA launchers (mpc_lane_inst.hip, mpc_ubg_inst.hip) ignore max_waves and
launch their full grid whatever the share says -- nothing here runs THEIR refill passes more than once per lane -- and the
three-wavefronts-per-SIMD build of the N = 10 hand-written kernel, which the launcher picks from 6 instances per lane of
the whole chip on.
"""
import numpy as np
import pytest

from conftest import bits_equal, bits_equal32
from test_group_gpu import BUILT as GROUP_BUILT, GROUP_ATOL
from test_groupg_gpu import ATOL as GROUPG_ATOL, BUILT as GROUPG_BUILT, GNAMES, _soa

pytestmark = pytest.mark.gpu

LANE_FMA, GROUP = 3, 4      # tpc_mpc_algo
WAVE = 64
NTHREADS = 16               # of the CPU references
GRIDS = [1, 3]              # wavefronts (3: n_waves is no power of two in the dealt indexing order[wl * n_waves + wave_id])
A_MAX = 22.0 * np.pi / 180.0
PHASES = [(0, 10000), (3, 10000), (50, 51), (50, 300)]   # (smo_iters, max_iter): fresh v after a carried one; every iteration
#                                                          ends in a refill pass; stops and caps in the same pass
BOUNDS = [((-0.3, -0.2), (0.25, 0.4), True), ((0.05, -0.3), (0.3, -0.1), False), ((-1e-3, -0.5), (2e-3, 0.5), True)]
# input streams whose instances nearly all enter the projected-gradient phase (counted with the CPU model, also under PHASES)
STREAM = {4: 200000, 5: 200000, 10: 900, 20: 3000}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def model():
    from tests.model.bindings import UbModel
    return UbModel()


@pytest.fixture(scope="module")
def model32():
    from tests.model.bindings import UbModel
    return UbModel("f32")


def _solver(H, algo, dtype="f64", G=0, **kw):
    from trajectory_controller_amd import MpcSolver, capi
    s = MpcSolver(horizon=H, device=0, dtype=dtype, algo=algo, **kw)
    if G:
        s.set_option(capi.OPT_GROUP_LANES, G)
    s.set_profiling(True)
    return s


def _pin(s, waves):
    """the persistent grid of this handle's solves: `waves` wavefronts (0: the whole chip again)"""
    s._check(s._lib.tpc_mpc_x_set_group_share(s._h, waves, 0))


def _sizes(L, tail, H=None, waves=None):
    sizes = [L - 1, L, L + 1, 4 * L, 4 * L + tail]
    if H is not None and H <= 10 and waves == 1:
        sizes.append(300)          # the multi-pass dealt queue
    return sizes


def _entered(n, L, ref_iters, smo):
    """Condition on the inputs: at the sizes of four grids' worth, at least two grids' worth of instances enter the
    projected-gradient phase -- every lane is refilled while its neighbours iterate."""
    if n >= 4 * L:
        entered = int((np.asarray(ref_iters) > smo).sum())
        assert entered >= 2 * L, f"n={n}: only {entered} instances enter the projected-gradient phase, the grid holds {L}"


def _refilled(s, n, L, wavefronts, what):
    if n >= 4 * L:
        wave_iters, refill_blocks = s.last_lane_stats()
        print(f"{what} n={n}: {wavefronts} wavefronts, {wave_iters} wave iterations, {refill_blocks} refill passes")
        assert refill_blocks > wavefronts, (n, refill_blocks)


def _compact_dev(torch, s, v, dy, dphi, expect):
    tdt = torch.float32 if v.dtype == np.float32 else torch.float64
    tv, ty, tp = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype=tdt) for a in (v, dy, dphi))
    f, r, it = s.solve_batch_compact(tv, ty, tp, want_iters=True)
    torch.cuda.synchronize()
    assert s.last_kernel_times()[2] == expect          # the family under test ran
    return f.cpu().numpy(), r.cpu().numpy(), it.cpu().numpy()


def _general_dev(torch, s, g, I, expect):
    dev = [torch.from_numpy(_soa(g[k])).to("cuda:0") for k in GNAMES]
    u0, it = s.solve_batch_general(*dev, inputs=I, want_iters=True)
    torch.cuda.synchronize()
    assert s.last_kernel_times()[2] == expect
    return u0.cpu().numpy().T, it.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# 1. LANE_FMA compact against the CPU model: bits and iteration counts

def _lane_grid(H, dtype, W):
    """(share to ask for, wavefronts in the grid it gives): fp32 at N = 10 / 20 launches workgroups of two wavefronts
    (UbPlan::occ) -- W = 1 asks for ONE wavefront and gets the smallest grid, one workgroup; W = 3 asks for three workgroups."""
    occ = 2 if dtype == "f32" and H in (10, 20) else 1
    return (W if occ == 1 or W == 1 else W * occ), W * occ


def _lane_fma_pinned(torch, mdl, H, W, inputs, dtype="f64", model_kw=None, solver_kw=None, hold_cap_flag=False,
                     after=None):
    """`inputs(n)` -> (v, dy, dphi): every size of the ladder on one handle with the grid pinned, each against the model."""
    from trajectory_controller_amd import FLAG_MAX_ITER
    model_kw, solver_kw = model_kw or {}, solver_kw or {}
    share, wavefronts = _lane_grid(H, dtype, W)
    L = WAVE * wavefronts
    smo, cap = solver_kw.get("smo_iters", 50), solver_kw.get("max_iter", 10000)
    eq = bits_equal32 if dtype == "f32" else bits_equal
    with _solver(H, "lane_fma", dtype, **solver_kw) as s:
        _pin(s, share)
        for n in _sizes(L, 37, H, W):
            v, dy, dphi = inputs(n)
            mf, mr, mit, _ = mdl.solve_compact(H, v, dy, dphi, nthreads=NTHREADS, smo_iters=smo, max_iter=cap,
                                               eps=solver_kw.get("eps", 0.01), **model_kw)
            _entered(n, L, mit, smo)
            f, r, it = _compact_dev(torch, s, v, dy, dphi, LANE_FMA)
            flags = s.last_flags
            assert np.array_equal(it, mit), n
            assert eq(f, mf) and eq(r, mr), n
            if hold_cap_flag:
                assert bool(flags & FLAG_MAX_ITER) == bool((mit == cap).any()), n
            _refilled(s, n, L, wavefronts, f"LANE_FMA {dtype} H={H}")
            if after is not None:
                after(n, (v, dy, dphi), (f, r, it), flags)


def _stream(H, dtype="f64", first=None):
    from trajectory_controller_amd.synth import compact_inputs
    first = STREAM[H] if first is None else first
    cast = np.float32 if dtype == "f32" else np.float64
    return lambda n: tuple(a.astype(cast) for a in compact_inputs(H, n, first=first))


def _mostly_entering(H, n, first, counts, smo=50):
    """The box that does not contain the start point ends nine instances in ten inside the coordinate-descent phase: no
    prefix of a stream refills much.  Three quarters of this batch are therefore the first instances of the stream that
    the reference takes INTO the projected-gradient phase (`counts(v, dy, dphi)` > smo_iters: a choice of inputs by the
    reference's iteration counts), one quarter the first that it does not, in the stream's order.  The exact build decides
    instance by instance, so the batch's reference is what the references below compute for it."""
    from trajectory_controller_amd.synth import compact_inputs
    pool = compact_inputs(H, 12 * n, first=first)
    it = counts(*pool)
    k = (3 * n + 3) // 4
    enter, rest = np.flatnonzero(it > smo), np.flatnonzero(it <= smo)
    assert len(enter) >= k and len(rest) >= n - k
    idx = np.sort(np.concatenate([enter[:k], rest[:n - k]]))
    return tuple(np.ascontiguousarray(a[idx]) for a in pool)


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("H", [4, 5, 10, 20])
def test_refill_lane_fma_f64(torch_cuda, model, H, W):
    """Default parameters.  N = 20 is the hand-written ub_pg_asm_kernel, N = 10 the SOLO build of the hand-written N = 10
    kernel, N = 4 / 5 the compiled kernel with its dealt queue."""
    _lane_fma_pinned(torch_cuda, model, H, W, _stream(H))


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("H", [4, 10, 20, 30, 40])
def test_refill_lane_fma_f32(torch_cuda, model32, H, W):
    """fp32 against UbModel("f32").  N = 10 / 20, W = 1: a share of one wavefront where a workgroup holds two -- the launcher
    rounds it UP to one workgroup (it used to launch a grid of zero: no solve, an invalid-configuration status)."""
    _lane_fma_pinned(torch_cuda, model32, H, W, _stream(H, "f32", first=200000), dtype="f32")


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("H,vmax,one_fast", [(20, 8.0, False), (20, 3.5, True), (10, 20.0, False), (10, 6.0, True)])
def test_refill_lane_fma_f32_stop_test_builds(torch_cuda, model32, H, vmax, one_fast, W):
    """The speed scalings of test_ub_gpu.py::test_ub_f32_stop_test_builds: beyond the rounding screen of the moved stop
    test, and one instance beyond it -- the MODE 1 (mask as arithmetic) build refills as well as the MODE 2 one."""
    base = _stream(H, "f32", first=300000)

    def inputs(n):
        v, dy, dphi = base(n)
        v = (v * np.float32(vmax / 4.0)).astype(np.float32)
        if one_fast:
            v[n // 2] = np.float32(4.0 * vmax)
        return v, dy, dphi
    _lane_fma_pinned(torch_cuda, model32, H, W, inputs, dtype="f32")


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("smo,cap", PHASES)
@pytest.mark.parametrize("H", [10, 20])
def test_refill_lane_fma_phase_boundaries(torch_cuda, model, H, smo, cap, W):
    """Coordinate-descent / projected-gradient hand-over and the iteration cap with refills: (0, .) gives every refilled
    lane a fresh v after it carried momentum, (50, 51) caps every instance after one projected-gradient iteration, (50, 300)
    mixes stops and caps in one pass.  FLAG_MAX_ITER follows the model's counts."""
    _lane_fma_pinned(torch_cuda, model, H, W, _stream(H), solver_kw=dict(smo_iters=smo, max_iter=cap), hold_cap_flag=True)


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("lo,hi,fast", BOUNDS)
@pytest.mark.parametrize("H", [10, 20])
def test_refill_lane_fma_other_bounds(torch_cuda, model, H, lo, hi, fast, W):
    """The compiled builds: unequal bounds (EQB = false, also at N = 10 / 20 where equal ones take the hand-written
    kernels), and the exact stop test for the box that does not contain the start point."""
    inputs = _stream(H)
    if not fast:
        inputs = lambda n: _mostly_entering(H, n, STREAM[H], lambda v, dy, dphi: model.solve_compact(
            H, v, dy, dphi, lo=lo, hi=hi, fast_stop=False, nthreads=NTHREADS)[2])
    _lane_fma_pinned(torch_cuda, model, H, W, inputs, model_kw=dict(lo=lo, hi=hi, fast_stop=fast),
                     solver_kw=dict(lower=lo, upper=hi))


@pytest.mark.parametrize("W", GRIDS)
def test_refill_lane_fma_exact_build_ended_by_the_cap(torch_cuda, model, W):
    """eps = 1e-13 is refused by the fast stop test's screen: the exact build, every instance through 1 450 iterations of it
    to the cap (tests/test_ub_gpu.py::test_ub_knobs_edges_and_exact_build's knobs)."""
    _lane_fma_pinned(torch_cuda, model, 10, W, _stream(10), model_kw=dict(fast_stop=False),
                     solver_kw=dict(eps=1e-13, max_iter=1500), hold_cap_flag=True)


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("weights", [None, (20.0, 0.0, 0.0005, 10.0)])
def test_refill_lane_fma_queue_is_not_the_batch_n20(torch_cuda, model, weights, W):
    """test_ub_cd_asm_gpu.py::test_cd_loop_mixed_screen_nonfinite_zero_qdiag_n20's poisoning, with refills: NaN and +-inf
    inputs in the first and the last wavefront of the batch (they fail the screen: the exact build runs, and they never enter
    the queue, so n_queue < n), one instance with v = 0 (done at once), and the parameter set with weight_phi = 0
    (Q_diag = 0).  The poisoned instances come back as zeros with zero iterations and raise FLAG_NONFINITE."""
    from trajectory_controller_amd import FLAG_NONFINITE
    H = 20
    base = _stream(H)
    mkw = dict(fast_stop=None) if weights is None else dict(fast_stop=None, weights=weights)
    skw = {} if weights is None else dict(zip(("weight_y", "weight_phi", "weight_steering_front", "weight_steering_rear"), weights))

    def poisoned(n):
        last = (n - 1) // WAVE * WAVE                     # first lane of the last wavefront of the batch
        return [5, min(last + 3, n - 1), min(last + 9, n - 2)]

    def inputs(n):
        v, dy, dphi = (a.copy() for a in base(n))
        a, b, c = poisoned(n)
        dy[a], v[b], dphi[c] = np.nan, np.inf, -np.inf
        v[n // 3] = 0.0
        return v, dy, dphi

    def after(n, inp, out, flags):
        f, r, it = out
        bad = poisoned(n)
        assert np.all(f[bad] == 0) and np.all(r[bad] == 0) and np.all(it[bad] == 0), n
        assert flags & FLAG_NONFINITE, n
    _lane_fma_pinned(torch_cuda, model, H, W, inputs, model_kw=mkw, solver_kw=skw, after=after)


def test_refill_lane_fma_queue_order_changes_nothing_n20(torch_cuda, model):
    """The order of the queue decides which lane gets what and nothing else: N = 20 on ONE wavefront with the table's key,
    lambda's, the model's own counts as the hint (longest first) and the reversed hint (shortest first) -- the model's bits
    and counts every time."""
    H, W = 20, 1
    L = WAVE * W
    inputs = _stream(H)
    with _solver(H, "lane_fma") as s:
        _pin(s, W)
        for n in _sizes(L, 37):
            v, dy, dphi = inputs(n)
            mf, mr, mit, _ = model.solve_compact(H, v, dy, dphi, nthreads=NTHREADS)
            _entered(n, L, mit, 50)
            longest_first = np.maximum(mit, 1).astype(np.int32)
            shortest_first = (longest_first.max() + 1 - longest_first).astype(np.int32)
            for key, hint in (("table", None), ("lambda", None), ("hint", longest_first), ("hint", shortest_first)):
                s.set_queue_key(key != "lambda")
                if hint is not None:
                    s.set_work_hint(hint)
                f, r, it = _compact_dev(torch_cuda, s, v, dy, dphi, LANE_FMA)
                assert s.last_queue_key() == key
                assert np.array_equal(it, mit), (n, key)
                assert bits_equal(f, mf) and bits_equal(r, mr), (n, key)
                _refilled(s, n, L, W, f"LANE_FMA f64 H={H} key={key}")


# ---------------------------------------------------------------------------------------------
# 2. GROUP compact against the oracle: identical iteration counts, |du| <= 1e-9, bound-sitting controls bit for bit

def _group_first(H, G):
    return STREAM[H] if H in STREAM else 610000 + 100 * H + G       # (N = 30 / 40: test_group_gpu.py's streams)


def _group_pinned(torch, oracle, H, G, W, lo=None, hi=None, one_lane=False, **knobs):
    """one_lane: the batch is one the screen refuses, solved by LANE_FMA's exact build on the same pinned grid -- that
    kernel holds 64 instances per wavefront, and the ladder of sizes is the one-lane families'."""
    from trajectory_controller_amd import FLAG_MAX_ITER
    from trajectory_controller_amd.synth import compact_inputs
    L, tail = (WAVE * W, 37) if one_lane else (WAVE // G * W, 5)
    smo, cap = knobs.get("smo_iters", 50), knobs.get("max_iter", 10000)
    box = {} if lo is None else dict(lo=lo, hi=hi)
    lo, hi = (lo, hi) if lo is not None else ((-A_MAX, -A_MAX), (A_MAX, A_MAX))
    with _solver(H, "group", G=G, **knobs, **({} if not box else dict(lower=lo, upper=hi))) as s:
        _pin(s, W)
        for n in _sizes(L, tail):
            if one_lane:
                v, dy, dphi = _mostly_entering(H, n, _group_first(H, G), lambda *a: oracle.solve_compact(
                    H, *a, nthreads=NTHREADS, **box, **knobs)[2], smo)
            else:
                v, dy, dphi = compact_inputs(H, n, first=_group_first(H, G))
            of, orr, oit = oracle.solve_compact(H, v, dy, dphi, nthreads=NTHREADS, **box, **knobs)
            _entered(n, L, oit, smo)
            f, r, it = _compact_dev(torch, s, v, dy, dphi, GROUP)
            assert bool(s.last_flags & FLAG_MAX_ITER) == bool((oit == cap).any()), n
            assert np.array_equal(it, oit), n
            assert max(np.abs(f - of).max(), np.abs(r - orr).max()) <= GROUP_ATOL, n
            assert np.array_equal((of == lo[0]) | (of == hi[0]), (f == lo[0]) | (f == hi[0])), n
            assert np.array_equal((orr == lo[1]) | (orr == hi[1]), (r == lo[1]) | (r == hi[1])), n
            _refilled(s, n, L, W, f"GROUP f64 H={H} G={G}")


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("H,G", GROUP_BUILT)
def test_refill_group(torch_cuda, oracle, H, G, W):
    _group_pinned(torch_cuda, oracle, H, G, W)


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("smo,cap", PHASES)
@pytest.mark.parametrize("G", [2, 4])
def test_refill_group_phase_boundaries(torch_cuda, oracle, G, smo, cap, W):
    _group_pinned(torch_cuda, oracle, 10, G, W, smo_iters=smo, max_iter=cap)


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("lo,hi,fast", BOUNDS)
@pytest.mark.parametrize("H,G", [(20, 4), (40, 8)])
def test_refill_group_other_bounds(torch_cuda, oracle, H, G, lo, hi, fast, W):
    """Unequal bounds; the box without the start point fails the screen and runs LANE_FMA's exact build (ub_exact_h*: fp64
    N = 40 has no other one-lane LANE_FMA kernel left) on the pinned grid."""
    _group_pinned(torch_cuda, oracle, H, G, W, lo=lo, hi=hi, one_lane=not fast)


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("H,G", [(10, 2), (20, 4), (40, 8)])
def test_refill_group_f32_pinned_equals_unpinned(torch_cuda, H, G, W):
    """fp32 GROUP has no pinned reference: the pinned grid returns the bits and counts of the same handle's whole-chip grid,
    which test_group_gpu.py::test_group_fp32_vs_float_typed_oracle bounds (its stream).  (N = 10 / 20, W = 1: the exact
    build behind it, launched every time and returning at once, is LANE_FMA's two-wavefront workgroup asked for one
    wavefront.)"""
    from trajectory_controller_amd.synth import compact_inputs
    L = WAVE // G * W
    with _solver(H, "group", "f32", G=G) as s:
        for n in _sizes(L, 5):
            v, dy, dphi = (a.astype(np.float32) for a in compact_inputs(H, n, first=300000))
            _pin(s, 0)
            f0, r0, it0 = _compact_dev(torch_cuda, s, v, dy, dphi, GROUP)
            _entered(n, L, it0, 50)
            _pin(s, W)
            f, r, it = _compact_dev(torch_cuda, s, v, dy, dphi, GROUP)
            assert np.array_equal(it, it0), n
            assert bits_equal32(f, f0) and bits_equal32(r, r0), n
            _refilled(s, n, L, W, f"GROUP f32 H={H} G={G}")


# ---------------------------------------------------------------------------------------------
# 3. GROUPG general against the oracle

def _general(H, G, I, n):
    from trajectory_controller_amd.synth import general_inputs
    return general_inputs(H, n, I=I, first=880000 + 10 * H + G)      # (test_groupg_gpu.py's streams)


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("I,H,G", [(2, h, g) for h, g in GROUPG_BUILT] + [(1, 20, 4), (1, 40, 8)])
def test_refill_groupg_cold(torch_cuda, oracle, I, H, G, W):
    torch = torch_cuda
    L = WAVE // G * W
    with _solver(H, "group", G=G) as s:
        _pin(s, W)
        for n in _sizes(L, 5):
            g = _general(H, G, I, n)
            ou0, _, oit = oracle.solve_general(I, H, *[g[k] for k in GNAMES], nthreads=NTHREADS)
            _entered(n, L, oit, 50)
            u0, it = _general_dev(torch, s, g, I, GROUP)
            assert np.array_equal(it, oit), n
            assert np.abs(u0 - ou0).max() <= GROUPG_ATOL, n
            assert np.array_equal((ou0 == g["lo"]) | (ou0 == g["hi"]), (u0 == g["lo"]) | (u0 == g["hi"])), n
            _refilled(s, n, L, W, f"GROUPG I={I} H={H} G={G}")


@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H,G", [(20, 8), (40, 4)])
def test_refill_groupg_state_in_and_out(torch_cuda, oracle, I, H, G, W):
    """The STATE kernels (behind LANE's coordinate-descent kernel; the whole batch is their queue): warm start from random
    controls and a random v, half of the boxes random as in test_groupg_gpu.py::test_groupg_state_in_and_out -- u0, the
    solved sequence, dlib's v and the iteration counts against the oracle."""
    L = WAVE // G * W
    with _solver(H, "group", G=G) as s:
        _pin(s, W)
        for n in _sizes(L, 5):
            g = _general(H, G, I, n)
            rng = np.random.default_rng(300 + H + I)
            cin = rng.uniform(-0.3, 0.3, size=(n, H, I))
            vin = rng.uniform(-0.3, 0.3, size=(n, H, I))
            g["lo"][::2] = -rng.uniform(0.02, 0.6, size=g["lo"][::2].shape)
            g["hi"][::2] = rng.uniform(0.02, 0.6, size=g["hi"][::2].shape)
            ou0, cout, oit, vout = oracle.solve_general(I, H, *[g[k] for k in GNAMES], controls_in=cin, v_in=vin, want_v=True,
                                                        nthreads=NTHREADS)
            _entered(n, L, oit, 50)
            controls, vstate = _soa(cin), _soa(vin)
            u0, it = s.solve_batch_general(*[_soa(g[k]) for k in GNAMES], controls=controls, v_state=vstate, inputs=I,
                                           want_iters=True)
            assert s.last_kernel_times()[2] == GROUP
            assert np.array_equal(it, oit), n
            assert np.abs(u0.T - ou0).max() <= GROUPG_ATOL, n
            assert np.abs(controls.T.reshape(n, H, I) - cout).max() <= GROUPG_ATOL, n
            assert np.abs(vstate.T.reshape(n, H, I) - vout).max() <= GROUPG_ATOL, n
            _refilled(s, n, L, W, f"GROUPG state I={I} H={H} G={G}")
