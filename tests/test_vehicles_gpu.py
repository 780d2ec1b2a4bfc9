"""`-m gpu`: every compact-form kernel OFF the reference controller's parameter set and in reverse.

Nearly every other GPU test runs the default vehicle (weights 20 / 7 / 0.0005 / 10, step_size 0.1, wheelbase 0.21, box
+-22 deg on both inputs) with v > 0, where a hard-coded 0.21, an |a| for a = T v, a wrong sign of the bound offsets
(dlt, cs0, cs1) or s0 used for s1 cannot show.  Here a cell is one vehicle of tests/model/vehicles.py x one horizon:
nine parameter sets -- negative wheelbase and step size, exchanged steering weights, weight_phi = 0, unequal bounds, a
box without u = 0 -- with 30 % of the speeds negative and one v = 0, in deliberately small, ragged batches (333
instances up to N = 20, 141 above).  tests/test_vehicles_host.py asserts what the criteria rest on.

The criteria are the project's existing ones, per family: LANE (both layouts), the generic kernel and fp32 LANE equal
the oracle's bits and counts; LANE_FMA equals the CPU model's bits and, like WAVE and GROUP, has the oracle's counts and
|du| <= 1e-9; fp32 WAVE / GROUP under the bounds of tests/test_parity_gpu.py / tests/test_group_gpu.py.

One cell is special: (no_phi, N = 5) meets a structural tie in dlib's arg-max (NOTEBOOK.md; vehicles.cd_ties finds the
instances with no solver in the loop: 5 of the 333).  There a tolerance family is held to the oracle on the other 328
and, LANE_FMA, to the model's bits on all; AUTO runs the bit-exact kernels for weight_phi = 0 and meets 1e-9 everywhere.
"""
import functools

import numpy as np
import pytest

from conftest import bits_equal, bits_equal32, load_golden
from tests.model import vehicles as vh

pytestmark = pytest.mark.gpu

WAVE, LANE, LANE_FMA, GROUP = 1, 2, 3, 4          # tpc_mpc_algo
GENERIC = 100                                     # what last_kernel_times names the any-horizon kernel (csrc/mpc_internal.h)
ATOL = 1e-9                                       # WAVE_ATOL, UB_ATOL, GROUP_ATOL
NTHREADS = 16
ALWAYS, NEVER = 1 << 40, 0                        # tpc_mpc_x_set_lanex_below: G lanes per instance / one lane
FINDING = ("no_phi", 5)
GROUP_BUILT = [(10, 2), (10, 4), (20, 2), (20, 4), (20, 8), (30, 2), (30, 4), (30, 8), (40, 2), (40, 4), (40, 8)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def test_constants_are_the_other_modules():
    from test_group_gpu import BUILT, GROUP_ATOL
    from test_parity_gpu import WAVE_ATOL
    from test_ub_gpu import UB_ATOL
    assert BUILT == GROUP_BUILT and GROUP_ATOL == WAVE_ATOL == UB_ATOL == ATOL


@functools.lru_cache(maxsize=None)
def _inputs(H, dtype="f64", n=None):
    cast = np.float32 if dtype == "f32" else np.float64
    out = tuple(np.ascontiguousarray(a.astype(cast)) for a in vh.inputs(H, n or vh.batch_size(H)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name, H, dtype="f64"):
    """(front, rear, iters) of the cell by the restatement typed `dtype`: computed once, shared, never modified"""
    from oracle.bindings import Oracle
    return Oracle(dtype).solve_compact(H, *_inputs(H, dtype), nthreads=NTHREADS, **vh.oracle_kw(name))


@functools.lru_cache(maxsize=None)
def _model(name, H, dtype="f64"):
    from tests.model.bindings import UbModel
    return UbModel(dtype).solve_compact(H, *_inputs(H, dtype), nthreads=NTHREADS, fast_stop=None, **vh.oracle_kw(name))


@functools.lru_cache(maxsize=None)
def _held(name, H):
    """the instances on which a tolerance family is held to dlib's path: all, but for the tied ones of the one cell"""
    n = vh.batch_size(H)
    if (name, H) != FINDING:
        return np.ones(n, dtype=bool)
    ties = vh.cd_ties(name, H, *_inputs(H))
    assert 0 < ties.sum() <= 5
    return ~ties


def _solve(torch, name, H, algo, dtype="f64", G=0, below=None, share=None, inputs=None, **over):
    """one solve of the cell on the device: (front, rear, iters, flags, family that ran, solver-side extras)"""
    from trajectory_controller_amd import MpcSolver, capi
    tdt = torch.float32 if dtype == "f32" else torch.float64
    tv, ty, tp = (torch.from_numpy(np.array(a)).to("cuda:0", dtype=tdt) for a in (inputs or _inputs(H, dtype)))
    with MpcSolver(horizon=H, device=0, dtype=dtype, algo=algo, **dict(vh.solver_kw(name), **over)) as s:
        if G:
            s.set_option(capi.OPT_GROUP_LANES, G)
        if below is not None:
            s._check(s._lib.tpc_mpc_x_set_lanex_below(s._h, below))
        if share is not None:
            s._check(s._lib.tpc_mpc_x_set_group_share(s._h, share, 0))
        s.set_profiling(True)
        f, r, it = s.solve_batch_compact(tv, ty, tp, want_iters=True)
        torch.cuda.synchronize()
        ran = s.last_kernel_times()[2]
        extra = dict(queue_key=s.last_queue_key(), lane_stats=s.last_lane_stats() if share is not None else None)
        return f.cpu().numpy(), r.cpu().numpy(), it.cpu().numpy(), s.last_flags, ran, extra


def _tolerance(name, H, f, r, it, what):
    """the tolerance families' statement against the oracle: identical counts, |du| <= 1e-9, bound-sitting controls
    bit for bit -- on the instances the cell holds to dlib's path"""
    of, orr, oit = _oracle(name, H)
    keep = _held(name, H)
    err = np.maximum(np.abs(f - of), np.abs(r - orr))
    print(f"{what} {name} H={H}: max |du| {err[keep].max():.2e}, counts differ in {int((it != oit)[keep].sum())} of {int(keep.sum())}"
          + ("" if keep.all() else f"; on the {int((~keep).sum())} tied: max |du| {err[~keep].max():.2e}, counts differ in {int((it != oit)[~keep].sum())}"))
    assert np.array_equal(it[keep], oit[keep])
    assert err[keep].max() <= ATOL
    lo, hi = vh.VEHICLES[name][3:]
    for j, (o, m) in enumerate(((of, f), (orr, r))):
        assert np.array_equal(((o == lo[j]) | (o == hi[j]))[keep], ((m == lo[j]) | (m == hi[j]))[keep])


# ---------------------------------------------------------------------------------------------
# LANE, both layouts, and the generic kernel: the oracle's bits

@pytest.mark.parametrize("name,H", vh.cells())
def test_lane_bits(torch_cuda, name, H):
    of, orr, oit = _oracle(name, H)
    for below in (ALWAYS, NEVER):                # (N = 4, 5 have one layout: the call is the same twice)
        f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "lane", below=below)
        assert ran == LANE
        assert np.array_equal(it, oit), below
        assert bits_equal(f, of) and bits_equal(r, orr), below


@pytest.mark.parametrize("name,H", vh.cells((10, 20)))
def test_lane_f32_bits(torch_cuda, name, H):
    of, orr, oit = _oracle(name, H, "f32")
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "lane", dtype="f32")
    assert ran == LANE and f.dtype == np.float32
    assert np.array_equal(it, oit) and bits_equal32(f, of) and bits_equal32(r, orr)


@pytest.mark.parametrize("H", vh.HORIZONS)
def test_lane_golden(torch_cuda, H):
    """the real-dlib fixtures of the family (tests/golden/make_golden_vehicles.py), both layouts"""
    g = load_golden(f"compact_vehicles_H{H}.npz")
    ins = (g["v"], g["dy"], g["dphi"])
    for name in vh.names_at(H):
        for below in (ALWAYS, NEVER):
            f, r, _, _, ran, _ = _solve(torch_cuda, name, H, "lane", below=below, inputs=ins)
            assert ran == LANE and bits_equal(f, g[f"front_{name}"]) and bits_equal(r, g[f"rear_{name}"]), (name, below)


@pytest.mark.parametrize("name,H,dtype", [(name, H, dtype) for H, dtype in ((7, "f64"), (33, "f64"), (7, "f32"))
                                          for name in vh.names_at(H)])
def test_generic_kernel_bits(torch_cuda, name, H, dtype):
    """horizons without specialised kernels (H as a run-time value), asked for through AUTO: that kernel ran, and its
    bits and counts are the oracle's"""
    from oracle.bindings import Oracle
    n = vh.batch_size(H)
    ins = _inputs(H, dtype, n)
    of, orr, oit = Oracle(dtype).solve_compact(H, *ins, nthreads=NTHREADS, **vh.oracle_kw(name))
    assert np.median(oit) >= 60 or name == "offset"
    eq = bits_equal32 if dtype == "f32" else bits_equal
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "auto", dtype=dtype, inputs=ins)
    assert ran == GENERIC
    assert np.array_equal(it, oit) and eq(f, of) and eq(r, orr)


# ---------------------------------------------------------------------------------------------
# WAVE

@pytest.mark.parametrize("name,H", vh.cells())
def test_wave(torch_cuda, name, H):
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "wave")
    assert ran == WAVE
    _tolerance(name, H, f, r, it, "WAVE")


@pytest.mark.parametrize("name", vh.names_at(10))
def test_wave_f32(torch_cuda, name):
    """tests/test_parity_gpu.py::test_wave_fp32_vs_float_typed_oracle's bounds at H = 10: the error quantiles and the
    floor of equal iteration counts, 0.8.  One vehicle takes that test's floor for LONGER solves instead: in fp32 the
    share of equal counts falls with the length of the solve (its floors are 0.9 / 0.8 / 0.4 at H = 5 / 10 / 20, where
    the default vehicle's median count is 113 / 240 / 722), and `short_fast` at H = 10 iterates longer than the default
    does at H = 20 (median 1032, tests/test_vehicles_host.py): 0.4.  Measured: 0.54 there, 0.92 .. 1.00 elsewhere."""
    H = 10
    of, orr, oit = _oracle(name, H, "f32")
    longer_than_default_h20 = np.median(_oracle(name, H)[2]) > np.median(_oracle("default", 20)[2])
    assert longer_than_default_h20 == (name == "short_fast")
    floor = 0.4 if longer_than_default_h20 else 0.8
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "wave", dtype="f32")
    same = float(np.mean(it == oit))
    err = np.maximum(np.abs(f - of), np.abs(r - orr))
    print(f"WAVE fp32 {name} H={H}: equal iteration counts {same:.4f}; |du| median {np.median(err):.2e} "
          f"p99 {np.quantile(err, 0.99):.2e} max {err.max():.2e}")
    assert ran == WAVE
    assert same >= floor and np.median(err) <= 2e-5 and np.quantile(err, 0.99) <= 5e-3


# ---------------------------------------------------------------------------------------------
# LANE_FMA

@pytest.mark.parametrize("name,H", vh.cells((4, 5, 10, 20)))
def test_lane_fma_f64(torch_cuda, name, H):
    """The CPU model's bits and counts (N = 20: the hand-written coordinate-descent and projected-gradient loops where
    the bounds are equal, the compiled builds for `asym`, the exact stop-test build for `offset` -- whichever the screens
    choose, the family ran), and the oracle's counts within 1e-9."""
    mf, mr, mit, _ = _model(name, H)
    f, r, it, _, ran, extra = _solve(torch_cuda, name, H, "lane_fma")
    assert ran == LANE_FMA
    assert np.array_equal(it, mit) and bits_equal(f, mf) and bits_equal(r, mr)
    _tolerance(name, H, f, r, it, "LANE_FMA")
    if H == 20:                                  # the table of predicted counts speaks about ONE parameter set
        assert extra["queue_key"] == ("table" if name == "default" else "lambda")


@pytest.mark.parametrize("name,H", vh.cells((4, 10, 20, 30, 40)))
def test_lane_fma_f32(torch_cuda, name, H):
    mf, mr, mit, _ = _model(name, H, "f32")
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "lane_fma", dtype="f32")
    assert ran == LANE_FMA
    assert np.array_equal(it, mit) and bits_equal32(f, mf) and bits_equal32(r, mr)


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("name", vh.names_at(20))
def test_lane_fma_n20_refills(torch_cuda, name, W):
    """N = 20 on the pinned grids of tests/test_refill_gpu.py: 64 / 192 lanes for 333 instances, so lanes are refilled
    while their neighbours iterate -- with a, c, the offsets and the two half-widths of another vehicle in the records."""
    H = 20
    mf, mr, mit, _ = _model(name, H)
    f, r, it, _, ran, extra = _solve(torch_cuda, name, H, "lane_fma", share=W)
    wave_iters, refill_blocks = extra["lane_stats"]
    print(f"LANE_FMA {name} N=20 on {W} wavefronts: {wave_iters} wave iterations, {refill_blocks} refill passes, key {extra['queue_key']}")
    assert ran == LANE_FMA
    assert np.array_equal(it, mit) and bits_equal(f, mf) and bits_equal(r, mr)
    assert extra["queue_key"] == ("table" if name == "default" else "lambda")
    if W == 1 and name != "offset":              # (4 grids' worth; `offset` ends most instances before the queue)
        assert int((mit > 50).sum()) >= 2 * 64 and refill_blocks > W


# ---------------------------------------------------------------------------------------------
# GROUP

@pytest.mark.parametrize("H,G", GROUP_BUILT)
def test_group(torch_cuda, H, G):
    for name in vh.names_at(H):
        f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "group", G=G)
        assert ran == GROUP, name
        _tolerance(name, H, f, r, it, f"GROUP G={G}")


@pytest.mark.parametrize("name", vh.names_at(20))
def test_group_f32(torch_cuda, name):
    """tests/test_group_gpu.py::test_group_fp32_vs_float_typed_oracle's statement at (20, 4)"""
    H, G = 20, 4
    of, orr, oit = _oracle(name, H, "f32")
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "group", dtype="f32", G=G)
    lf, lr, lit, _, lran, _ = _solve(torch_cuda, name, H, "lane_fma", dtype="f32")
    err = np.maximum(np.abs(f - of), np.abs(r - orr))
    same, same_l = float(np.mean(it == oit)), float(np.mean(it == lit))
    print(f"fp32 GROUP {name} H={H} G={G}: equal iteration counts vs restatement {same:.4f}, vs LANE_FMA {same_l:.4f}, "
          f"median |du| {np.median(err):.2e}, p99 {np.quantile(err, 0.99):.2e}")
    lo, hi = (np.float32(b) for b in vh.VEHICLES[name][3]), (np.float32(b) for b in vh.VEHICLES[name][4])
    assert ran == GROUP and lran == LANE_FMA
    assert np.isfinite(f).all() and np.isfinite(r).all() and it.max() <= 10000
    for x, l_, h_ in zip((f, r), lo, hi):            # the box, and dlib's untouched start 0 where a solve ends at once
        assert x.min() >= min(l_, 0) and x.max() <= max(h_, 0)
    assert same >= 0.4 and same_l >= 0.4 and np.median(err) <= 1e-4


# ---------------------------------------------------------------------------------------------
# AUTO, the mixed entry, solve_one

@pytest.mark.parametrize("name", vh.names_at(20))
def test_auto_n20(torch_cuda, name):
    H = 20
    of, orr, oit = _oracle(name, H)
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "auto")
    err = max(np.abs(f - of).max(), np.abs(r - orr).max())
    print(f"AUTO {name} H={H} n={len(f)}: family {ran}, max |du| {err:.2e}")
    assert ran == (LANE if name == "no_phi" else WAVE)       # 333 instances: WAVE's; weight_phi = 0: the bit-exact kernels
    assert np.array_equal(it, oit) and err <= ATOL


@pytest.mark.parametrize("H,n", [(5, 3000), (4, 333), (10, 333)])
def test_auto_meets_its_guarantee_where_dlibs_arg_max_ties(torch_cuda, H, n):
    """weight_phi = 0 in reverse -- at N = 5 the batch on which 56 of 3000 LANE_FMA counts leave dlib's (tests/
    test_vehicles_host.py): AUTO runs LANE and returns dlib's bits; LANE_FMA named is taken at its word and returns
    the CPU model's."""
    from oracle.bindings import Oracle
    from tests.model.bindings import UbModel
    name = "no_phi"
    ins = vh.inputs(H, n, reverse_only=True, first=31000)
    of, orr, oit = Oracle().solve_compact(H, *ins, nthreads=NTHREADS, **vh.oracle_kw(name))
    mf, mr, mit, _ = UbModel().solve_compact(H, *ins, nthreads=NTHREADS, fast_stop=None, **vh.oracle_kw(name))
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "auto", inputs=ins)
    assert ran == LANE
    assert np.array_equal(it, oit) and max(np.abs(f - of).max(), np.abs(r - orr).max()) <= ATOL
    assert bits_equal(f, of) and bits_equal(r, orr)
    f, r, it, _, ran, _ = _solve(torch_cuda, name, H, "lane_fma", inputs=ins)
    assert ran == LANE_FMA
    assert np.array_equal(it, mit) and bits_equal(f, mf) and bits_equal(r, mr)
    if H == 5:
        assert int((mit != oit).sum()) == 56
    # fp32 is outside AUTO's guarantee and keeps its fast families
    f32 = _solve(torch_cuda, name, H, "auto", dtype="f32", inputs=tuple(a.astype(np.float32) for a in ins))
    assert f32[4] != LANE


# ---------------------------------------------------------------------------------------------
# AUTO's routing of tie-prone requests (csrc/tpc_mpc_api.cpp: cd_tie_prone, compact_algo) in every compact entry

def _reversed_no_phi(H, n):
    from oracle.bindings import Oracle
    ins = vh.inputs(H, n, reverse_only=True, first=31000)
    return ins, Oracle().solve_compact(H, *ins, nthreads=NTHREADS, **vh.oracle_kw("no_phi"))


@pytest.mark.parametrize("wphi,ran_want", [(0.0, LANE), (1e-20, LANE), (20.0 * 2.0 ** -30, LANE), (1e-3, WAVE)])
def test_auto_routing_threshold(torch_cuda, wphi, ran_want):
    """weight_phi <= 2^-30 weight_y is "zero" (a ratio of 5e-22 ties like 0 does, tests/test_vehicles_host.py); 1e-3 is
    not, and keeps the family the batch size asks for.  Either way: the oracle's counts within 1e-9."""
    from oracle.bindings import Oracle
    H, n = 5, 333
    ins = vh.inputs(H, n, reverse_only=True, first=31000)
    w = (20.0, wphi, 0.0005, 10.0)
    of, orr, oit = Oracle().solve_compact(H, *ins, nthreads=NTHREADS, **dict(vh.oracle_kw("no_phi"), weights=w))
    f, r, it, _, ran, _ = _solve(torch_cuda, "no_phi", H, "auto", inputs=ins, weight_phi=wphi)
    assert ran == ran_want
    assert np.array_equal(it, oit) and max(np.abs(f - of).max(), np.abs(r - orr).max()) <= ATOL


@pytest.mark.parametrize("path", ["resident", "resident_host", "launch", "host_option"])
def test_solve_one_on_the_traced_tie(torch_cuda, path):
    """The traced instance and the most parted one (tests/test_vehicles_host.py), on which the LANE_FMA arithmetic (and with it the host path) leaves dlib's path: under AUTO
    tpc_mpc_solve_one answers with dlib's bits and count on each of its GPU paths -- a LANE launch, not the resident
    wavefront -- and with TPC_MPC_OPT_HOST_SOLVE_ONE set, which a GPU handle must not follow here.  LANE_FMA named
    with that option is taken at its word: the CPU model's bits."""
    from oracle.bindings import Oracle
    from test_abi_gpu import _solve_one_paths
    from tests.model.bindings import UbModel
    from trajectory_controller_amd import MpcSolver, capi
    from test_vehicles_host import PARTED, TRACED
    H = 5
    kw = vh.oracle_kw("no_phi")
    with MpcSolver(horizon=H, device=0, algo="auto", **vh.solver_kw("no_phi")) as s:
        if path == "host_option":
            s.set_option(capi.OPT_HOST_SOLVE_ONE, 10)
        else:
            _solve_one_paths(s, capi, path)
        s.set_profiling(True)
        for (v, dy, dphi), apart in ((TRACED, 0.0), (PARTED, 1e-3), (TRACED, 0.0)):
            of, orr, oit = Oracle().solve_compact(H, [v], [dy], [dphi], **kw)
            mf, mr, mit, _ = UbModel().solve_compact(H, [v], [dy], [dphi], fast_stop=None, **kw)
            assert mit[0] != oit[0] and max(abs(mf[0] - of[0]), abs(mr[0] - orr[0])) >= apart     # it does part the two
            f, r = s.solve_one(v, dy, dphi)
            assert bits_equal([f, r], [of[0], orr[0]])
            assert s.last_solve_one_flags() == (0, int(oit[0]))
            assert s.last_kernel_times()[2] == LANE
            if path == "host_option":
                f, r = s.solve_one(v, dy, dphi, algo=capi.ALGO_LANE_FMA)
                assert bits_equal([f, r], [mf[0], mr[0]]) and s.last_solve_one_flags() == (0, int(mit[0]))


def test_mixed_entry_routes_tie_prone_bins_to_lane(torch_cuda):
    """no_phi under AUTO through the mixed entry, every speed reversed (the N = 5 bin holds parted instances): every
    bin comes back with the oracle's bits -- group_applicable and the bins' own solves follow compact_algo."""
    from tests.model.bindings import UbModel
    from trajectory_controller_amd import MpcSolver
    torch = torch_cuda
    Hs, per = (5, 10, 20, 40), 150
    parts = [_reversed_no_phi(H, per) for H in Hs]
    mit5 = UbModel().solve_compact(5, *parts[0][0], nthreads=NTHREADS, fast_stop=None, **vh.oracle_kw("no_phi"))[2]
    assert (mit5 != parts[0][1][2]).sum() >= 2
    v, dy, dphi = (np.concatenate([p[0][c] for p in parts]) for c in range(3))
    hz = np.repeat(np.array(Hs, dtype=np.int32), per)
    perm = np.random.default_rng(12).permutation(len(hz))
    tv, ty, tp = (torch.from_numpy(np.ascontiguousarray(a[perm])).to("cuda:0") for a in (v, dy, dphi))
    with MpcSolver(horizon=20, device=0, algo="auto", **vh.solver_kw("no_phi")) as s:
        f, r, it = s.solve_batch_compact_mixed(torch.from_numpy(hz[perm]).to("cuda:0"), tv, ty, tp, want_iters=True)
        torch.cuda.synchronize()
    inv = np.argsort(perm)
    f, r, it = f.cpu().numpy()[inv], r.cpu().numpy()[inv], it.cpu().numpy()[inv]
    for b, H in enumerate(Hs):
        sl = slice(b * per, (b + 1) * per)
        of, orr, oit = parts[b][1]
        assert np.array_equal(it[sl], oit) and bits_equal(f[sl], of) and bits_equal(r[sl], orr), H


@pytest.mark.parametrize("H", [5, 20])
def test_follow_batch_routes_tie_prone_requests_to_lane(torch_cuda, H):
    """follow_batch with no_phi's parameters under AUTO: the oracle's counts and bits on the entry's own targets, and
    the family that ran is LANE."""
    from oracle.bindings import Oracle
    from test_follow_gpu import _batch, _compose_compact, _crossing, _dev, _np, _solver, _table
    torch = torch_cuda
    b = _batch("random", 333)
    dev = _dev(torch, b)
    lookup, tab = _table(torch, "four")
    with _solver(H, "auto", **vh.solver_kw("no_phi")) as s:
        s.set_profiling(True)
        f, r, ts, td, it = s.follow_batch(*dev, lookup=lookup, want_iters=True)
        torch.cuda.synchronize()
        assert s.last_kernel_times()[2] == LANE
        f, r, ts, it = _np(f, r, ts, it)
        _, _, _, _, v, tg = _compose_compact(torch, s, b, dev, lookup, tab)
    of, orr, oit = Oracle().solve_compact(H, v, tg[0], tg[1], nthreads=NTHREADS, **vh.oracle_kw("no_phi"))
    of, orr = _crossing(ts, of, orr)
    assert np.array_equal(it, oit) and bits_equal(f, of) and bits_equal(r, orr) and np.any(f != 0)


@pytest.mark.parametrize("algo", ["auto", "lane"])
@pytest.mark.parametrize("name", ["asym", "neg_l"])
def test_mixed_entry(torch_cuda, name, algo):
    """Horizons 5 / 10 / 20 / 40, 150 instances each, interleaved: per bin the oracle's counts and <= 1e-9 under AUTO, its
    bits under LANE."""
    from oracle.bindings import Oracle
    from trajectory_controller_amd import MpcSolver
    torch = torch_cuda
    Hs, per = (5, 10, 20, 40), 150
    parts = [vh.inputs(H, per) for H in Hs]
    v, dy, dphi = (np.concatenate([p[c] for p in parts]) for c in range(3))
    hz = np.repeat(np.array(Hs, dtype=np.int32), per)
    perm = np.random.default_rng(11).permutation(len(hz))
    tv, ty, tp = (torch.from_numpy(np.ascontiguousarray(a[perm])).to("cuda:0") for a in (v, dy, dphi))
    with MpcSolver(horizon=20, device=0, algo=algo, **vh.solver_kw(name)) as s:
        f, r, it = s.solve_batch_compact_mixed(torch.from_numpy(hz[perm]).to("cuda:0"), tv, ty, tp, want_iters=True)
        torch.cuda.synchronize()
    inv = np.argsort(perm)
    f, r, it = f.cpu().numpy()[inv], r.cpu().numpy()[inv], it.cpu().numpy()[inv]
    for b, H in enumerate(Hs):
        sl = slice(b * per, (b + 1) * per)
        of, orr, oit = Oracle().solve_compact(H, *parts[b], nthreads=NTHREADS, **vh.oracle_kw(name))
        assert np.array_equal(it[sl], oit), H
        if algo == "lane":
            assert bits_equal(f[sl], of) and bits_equal(r[sl], orr), H
        else:
            assert max(np.abs(f[sl] - of).max(), np.abs(r[sl] - orr).max()) <= ATOL, H


@pytest.mark.parametrize("path", ["resident", "resident_host", "launch"])
@pytest.mark.parametrize("H", [4, 5, 20])
@pytest.mark.parametrize("name", ["neg_l", "asym", "rear_cheap"])
def test_solve_one(torch_cuda, name, H, path):
    """tpc_mpc_solve_one on its three GPU paths (tests/test_abi_gpu.py::_solve_one_paths), six inputs of both signs"""
    from test_abi_gpu import _solve_one_paths
    from trajectory_controller_amd import MpcSolver, capi
    v, dy, dphi = _inputs(H)
    of, orr, oit = _oracle(name, H)
    ks = list(np.flatnonzero(v < 0)[:3]) + list(np.flatnonzero(v > 0)[:3])
    with MpcSolver(horizon=H, device=0, algo="auto", **vh.solver_kw(name)) as s:
        _solve_one_paths(s, capi, path)
        for k in ks:
            f, r = s.solve_one(float(v[k]), float(dy[k]), float(dphi[k]))
            flags, it = s.last_solve_one_flags()
            assert abs(f - of[k]) <= ATOL and abs(r - orr[k]) <= ATOL, k
            assert it == oit[k] and flags == 0, k


# ---------------------------------------------------------------------------------------------
# the raw-trajectory entries with another vehicle's step_size / wheelbase / weights

@pytest.mark.parametrize("family", ["lane", "auto"])
@pytest.mark.parametrize("H", [4, 20])
@pytest.mark.parametrize("name", ["neg_l", "long_slow"])
def test_follow_entries(torch_cuda, name, H, family):
    """tests/test_follow_gpu.py's criteria on fr.random_batch: follow_batch is, bit for bit, the compact solve of its
    own device targets (LANE: the oracle's bits with the vehicle's parameters); follow_batch_horizon's default spacing
    is speed x THIS solver's step_size -- its targets equal tests/model/follow_ref.py's -- and it is the general solve
    of its own targets on the model built from this step_size and wheelbase."""
    from oracle.bindings import Oracle
    from test_follow_gpu import (PHI_TOL, TRAJ, _batch, _compose_compact, _crossing, _dev, _general_arrays, _np,
                                 _solver, _table)
    from tests.model import follow_ref as fr
    torch = torch_cuda
    T = vh.VEHICLES[name][1]
    b = _batch("random", 333)
    n = len(b["count"])
    dev = _dev(torch, b)
    lookup, tab = _table(torch, "four")
    with _solver(H, family, **vh.solver_kw(name)) as s:
        f, r, ts, td, it = s.follow_batch(*dev, lookup=lookup, want_iters=True)
        flags = s.last_flags
        f, r, ts, it = _np(f, r, ts, it)
        wf, wr, wit, wflags, v, tg = _compose_compact(torch, s, b, dev, lookup, tab)
        assert np.array_equal(it, wit) and flags == wflags
        assert bits_equal(f, wf) and bits_equal(r, wr) and np.any(f != 0)
        if family == "lane":
            of, orr, oit = Oracle().solve_compact(H, v, tg[0], tg[1], nthreads=NTHREADS, **vh.oracle_kw(name))
            of, orr = _crossing(ts, of, orr)
            assert np.array_equal(it, oit) and bits_equal(f, of) and bits_equal(r, orr)
        # the horizon entry, default spacing
        f, r, ts, td, tg, it = s.follow_batch_horizon(*dev, lookup=lookup, want_targets=True, want_iters=True)
        flags = s.last_flags
        host, gen = _general_arrays(torch, s, b, tab)
        u0, wit = s.solve_batch_general(*gen, tg, inputs=2, want_iters=True)
        wflags = s.last_flags
    f, r, ts, it, u0, wit, tg = _np(f, r, ts, it, u0, wit, tg)
    spacing = fr.default_spacing(fr.lut_batch(b["carv"], *tab), T)
    want = fr.targets_of(fr.horizon_batch(*[b[k] for k in TRAJ], b["count"], b["look"], spacing, H, None))
    assert bits_equal(tg[0::2], want[0::2]) and np.abs(tg[1::2] - want[1::2]).max() <= PHI_TOL
    wf, wr = _crossing(ts, u0[0], u0[1])
    assert np.array_equal(it, wit) and flags == wflags
    assert bits_equal(f, wf) and bits_equal(r, wr) and np.any(f != 0)
    if family == "lane":
        ou0, _, oit = Oracle().solve_general(2, H, *[a.T for a in host], tg.T.reshape(n, H, 2), nthreads=NTHREADS)
        of, orr = _crossing(ts, ou0[:, 0], ou0[:, 1])
        assert np.array_equal(it, oit) and bits_equal(f, of) and bits_equal(r, orr)


# ---------------------------------------------------------------------------------------------
# the exact compact entries: the device against the host-only handle (held to the general entries on the CPU)

@pytest.mark.parametrize("device_arrays", [False, True], ids=["host_arrays", "device_arrays"])
@pytest.mark.parametrize("H", [5, 20])
@pytest.mark.parametrize("name", ["neg_l", "asym"])
def test_exact_compact_entries(torch_cuda, name, H, device_arrays):
    from test_vehicles_host import exact_entries
    torch = torch_cuda
    want = exact_entries(name, H, None)
    got = exact_entries(name, H, 0, torch if device_arrays else None)
    assert want.keys() == got.keys()
    for k in want:
        assert want[k].dtype == got[k].dtype and want[k].tobytes() == got[k].tobytes(), k
