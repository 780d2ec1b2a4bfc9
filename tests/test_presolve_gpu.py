"""`-m gpu` tests of AUTO's presolve on every route that reaches it (csrc/tpc_mpc_api.cpp: presolve_begin / presolve_finish /
general_launch; csrc/tpc_mpc_mixed.hip; csrc/mpc_sort.hip: presolve_merge*; csrc/mpc_lane.h: SUBSET 1 / 2).

AUTO promises that every instance a tolerance family leaves on max_iter comes back with dlib's bits.  At N = 40 most of
that work is done ahead of the tolerance family, on a side stream and a share of the chip, for the instances a
prediction names (lambda >= (max_iter / 7)^2); their results are merged over GROUP's, and the flag-driven second pass
skips them.  The cases (tests/model/presolve_cases.py, held to the oracle on the CPU by tests/test_presolve_host.py):
the queue fits / overflows what the side kernel takes, the general form through general_launch (the sharded entry on a
world of one; also as a block of a wider batch) and through tpc_mpc_solve_batch_general, the mixed entry's deferred presolve, no iteration counts wanted, instances that end on the cap inside the coordinate-descent
phase, two handles at once -- and what the presolve must NOT change.

Checked everywhere (test_capped_gpu.py's assertions): iteration counts equal the oracle's, capped instances equal it bit
for bit, everything else is within 1e-9, FLAG_MAX_ITER is raised exactly when something capped.  The library reports no
queue length; the evidence that a merge happened is the SPARE instances -- predicted, but converged after all: the
second pass never touches them, so only a merge can have put dlib's bits there; where the queue overflowed they keep
the tolerance family's bits.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal
from tests.model import presolve_cases as pc

pytestmark = pytest.mark.gpu

WAVE, LANE, LANE_FMA, GROUP = 1, 2, 3, 4
ATOL = 1e-9
SENT = -777.25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


_solved = {}


def _case(oracle, name):
    """The oracle's answer for a case, computed once per module and never written to."""
    if name not in _solved:
        _solved[name] = pc.solve_case(oracle, name)
    return _solved[name]


def _inputs(name):
    return pc.CASES[name]["inputs"](), pc.CASES[name]["knobs"]


def _differs(a, b):
    """Per instance (first axis): do the bit patterns differ?  (any NaN equals any NaN, as in conftest.bits_equal)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    d = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return d.reshape(len(d), -1).any(axis=1)


def _wrong_bits(s, out):
    d = np.zeros(s.n, dtype=bool)
    for a, b in zip(out, s.out):
        d |= _differs(a, b)
    return d


def _common(s, out, it, flags, label=""):
    """The common assertions for one batch (or one bin): `out` = the outputs in the order of s.out; it = None where no
    iteration counts were asked for; flags = None where the flag word describes more than this batch."""
    from trajectory_controller_amd import FLAG_MAX_ITER
    if it is not None:
        assert np.array_equal(it, s.oit), (label, int((it != s.oit).sum()))
    wrong = _wrong_bits(s, out)
    assert not (wrong & s.capped).any(), (label, "capped instances off dlib's bits", int((wrong & s.capped).sum()),
                                          "of", int(s.capped.sum()))
    for a, b in zip(out, s.out):
        assert np.abs(np.asarray(a) - b).max() <= ATOL, label
    if flags is not None:
        assert bool(flags & FLAG_MAX_ITER) == bool(s.capped.any()), (label, flags)


def _spare_merged(s, out, label=""):
    wrong = _wrong_bits(s, out)
    assert s.spare.any() and not (wrong & s.spare).any(), (label, "spare instances off dlib's bits: no merge?",
                                                           int((wrong & s.spare).sum()), "of", int(s.spare.sum()))


def _spare_not_merged(s, out, label=""):
    """The queue overflowed: the spare instances are the tolerance family's (within 1e-9 by _common), not dlib's bits"""
    assert s.spare.any()
    assert not all(bits_equal(a[s.spare], b[s.spare]) for a, b in zip(out, s.out)), label


def _route(torch, s, fits):
    """The case's precondition on THIS device: a partition of the chip fails here instead of testing the other route."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    limit, taken = pc.solo_limit(cu), int(s.taken.sum())
    assert s.n <= pc.batch_bound(cu), f"{cu} CUs: no presolve is tried for {s.n} instances (bound {pc.batch_bound(cu)})"
    if fits:
        assert taken <= limit, f"{cu} CUs: the predicted set ({taken}) does not fit the side kernel's one round ({limit})"
    else:
        assert taken > limit, f"{cu} CUs: the predicted set ({taken}) fits the side kernel's one round ({limit}): no overflow"


def _dev(torch, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)


def _np(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _compact_on(torch, solver, x, want_iters=True, expect=GROUP, **over):
    """(front, rear, iters or None, flags) of one compact solve on an open handle"""
    res = solver.solve_batch_compact(*x, want_iters=want_iters, **over)
    torch.cuda.synchronize()
    if expect is not None:
        assert solver.last_kernel_times()[2] == expect
    f, r = _np(*res[:2])
    return f, r, (res[2].cpu().numpy() if want_iters else None), solver.last_flags


def _auto(knobs, H=40, algo="auto", **kw):
    from trajectory_controller_amd import MpcSolver
    s = MpcSolver(horizon=H, device=0, algo=algo, **knobs, **kw)
    s.set_profiling(True)
    return s


def test_compact_overflow_then_fits_on_one_handle(torch_cuda, oracle):
    """A predicted set longer than the side kernel's one round (it returns at once, nothing is merged, the second pass
    skips nothing), one that fits, and the long one again, on ONE handle: a stale queue length, a presolve left marked
    busy or regrown scratch would show in the second or third solve."""
    torch = torch_cuda
    big, fit = _case(oracle, "overflow"), _case(oracle, "fits")
    _route(torch, big, fits=False)
    _route(torch, fit, fits=True)
    (xb, knobs), (xf, _) = _inputs("overflow"), _inputs("fits")
    xb, xf = _dev(torch, *xb), _dev(torch, *xf)
    with _auto(knobs) as s:
        f1, r1, it1, fl1 = _compact_on(torch, s, xb)
        f2, r2, it2, fl2 = _compact_on(torch, s, xf)
        f3, r3, it3, fl3 = _compact_on(torch, s, xb)
    _common(big, (f1, r1), it1, fl1, "overflow")
    _spare_not_merged(big, (f1, r1), "overflow")
    _common(fit, (f2, r2), it2, fl2, "fits")
    _spare_merged(fit, (f2, r2), "fits")
    _common(big, (f3, r3), it3, fl3, "overflow again")
    _spare_not_merged(big, (f3, r3), "overflow again")
    assert bits_equal(f3, f1) and bits_equal(r3, r1) and np.array_equal(it3, it1)


def test_want_iters_off(torch_cuda, oracle):
    """No iteration counts wanted: the handle's own buffer is the merge's target and the second pass's selector."""
    torch = torch_cuda
    for name, fits in (("fits", True), ("overflow", False)):
        s = _case(oracle, name)
        _route(torch, s, fits)
        x, knobs = _inputs(name)
        x = _dev(torch, *x)
        with _auto(knobs) as h:
            f0, r0, _, fl0 = _compact_on(torch, h, x, want_iters=False)
        with _auto(knobs) as h:
            f1, r1, it1, fl1 = _compact_on(torch, h, x, want_iters=True)
        _common(s, (f1, r1), it1, fl1, name)
        _common(s, (f0, r0), None, fl0, name + ", no iters")
        (_spare_merged if fits else _spare_not_merged)(s, (f0, r0), name + ", no iters")
        assert bits_equal(f0, f1) and bits_equal(r0, r1), name


def test_presolve_leaves_the_rest_alone(torch_cuda, oracle):
    """With the guarantee switched off there is no presolve and GROUP has the whole chip; with it, 9 / 16 of it: the
    instances the guarantee does not concern come back with the same bits, and every iteration count is the same."""
    from trajectory_controller_amd import capi
    torch = torch_cuda
    s = _case(oracle, "fits")
    _route(torch, s, fits=True)
    x, knobs = _inputs("fits")
    x = _dev(torch, *x)
    with _auto(knobs) as h:
        f, r, it, fl = _compact_on(torch, h, x)
    with _auto(knobs, options=capi.PARAM_FAST_CAPPED) as h:
        f2, r2, it2, _ = _compact_on(torch, h, x)
    _common(s, (f, r), it, fl, "fits")
    rest = ~s.taken & ~s.capped
    assert rest.any() and bits_equal(f[rest], f2[rest]) and bits_equal(r[rest], r2[rest])
    assert np.array_equal(it, it2)
    # (and switched off, the capped instances are NOT all dlib's bits: the comparison above is not of two equal routes)
    assert not (bits_equal(f2[s.capped], s.out[0][s.capped]) and bits_equal(r2[s.capped], s.out[1][s.capped]))


@pytest.mark.parametrize("name", ["cd_capped", "cd_capped_past"])
def test_cd_capped_instances_keep_the_guarantee(torch_cuda, oracle, name):
    """smo_iters >= max_iter: every instance ends inside the coordinate-descent phase, most of them on the cap.  Such an
    instance is never queued for the projected-gradient kernels, so a presolve that took it by prediction has nothing to
    merge for it -- and the second pass must not skip it on the strength of that prediction.

    Before presolve_lambda_impl switched the presolve off for smo_iters >= max_iter, AUTO returned GROUP's bits for the
    capped instances the prediction had taken: 2 588 of 2 615 (cd_capped) and 2 642 of 2 669 (cd_capped_past) differed
    from dlib, none of the 1 248 / 1 427 capped ones it had not taken."""
    torch = torch_cuda
    s = _case(oracle, name)
    _route(torch, s, fits=True)
    x, knobs = _inputs(name)
    with _auto(knobs) as h:
        f, r, it, fl = _compact_on(torch, h, _dev(torch, *x))
    wrong = _wrong_bits(s, (f, r))
    report = (f"{name}: capped and taken: {int((wrong & s.capped & s.taken).sum())} of {int((s.capped & s.taken).sum())} "
              f"off dlib's bits; capped and not taken: {int((wrong & s.capped & ~s.taken).sum())} of "
              f"{int((s.capped & ~s.taken).sum())}")
    print(report)
    assert np.array_equal(it, s.oit), report
    assert not (wrong & s.capped).any(), report
    _common(s, (f, r), it, fl, name)


def _general_call(solver, torch, I, n_full, k0, n, arrays, want_iters=True, sharded=True):
    """The general form on columns [k0, k0+n) of device arrays [comps, n_full] through the raw C entries: shifted base
    pointers, ld = n_full; outputs and iteration counts pre-filled with sentinels.  sharded: the sharded entry on a handle
    without a communicator (a world of one: its block is the whole call) -- the entry that goes through general_launch;
    else tpc_mpc_solve_batch_general.  Returns (u0[I, n_full], iters[n_full] or None, flags, family)."""
    from trajectory_controller_amd import capi
    u0 = torch.from_numpy(np.full((I, n_full), SENT)).cuda()
    iters = torch.from_numpy(np.full(n_full, -5, dtype=np.int32)).cuda() if want_iters else None
    ptr = lambda a: a.data_ptr() + k0 * 8
    io = capi.GeneralIO(inputs=I, n=n, ld=n_full, A=ptr(arrays[0]), B=ptr(arrays[1]), C=ptr(arrays[2]),
                        Q=ptr(arrays[3]), R=ptr(arrays[4]), lower=ptr(arrays[5]), upper=ptr(arrays[6]),
                        x0=ptr(arrays[7]), targets=ptr(arrays[8]), controls_inout=None, v_inout=None, u0=ptr(u0),
                        iters=iters.data_ptr() + 4 * k0 if want_iters else None)
    flags = C.c_uint32(0)
    torch.cuda.synchronize()
    lib, args = solver._lib, (solver._h, C.byref(solver.params), C.byref(io), C.byref(flags))
    if sharded:
        solver._check(lib.tpc_mpc_solve_batch_general_sharded(*args, None))
    else:
        solver._check(lib.tpc_mpc_solve_batch_general(*args, capi.DEVICE, None))
    torch.cuda.synchronize()
    family = solver.last_kernel_times()[2]
    return u0.cpu().numpy(), (iters.cpu().numpy() if want_iters else None), flags.value, family


def _general_dev(torch, g, n):
    return [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).to("cuda:0") for k in pc.GEN_NAMES]


@pytest.mark.parametrize("name", ["general_I1", "general_I2", "general_I2_default"])
def test_general_form_presolve(torch_cuda, oracle, name):
    """The general form's presolve (general_launch): per-instance models through lane_cd_kernel<SUBSET 2>, the SOLO
    lanexg kernel and the row-wise merge.  Of the public entries only tpc_mpc_solve_batch_general_sharded goes through
    general_launch; tpc_mpc_solve_batch_general launches on its own, without a presolve (its capped instances are all the
    second pass's): the first is held to the merge's evidence, the second to the guarantee alone."""
    torch = torch_cuda
    s = _case(oracle, name)
    _route(torch, s, fits=True)
    g, knobs = _inputs(name)
    I, n = pc.CASES[name]["I"], s.n
    dev = _general_dev(torch, g, n)
    with _auto(knobs) as h:
        u0, it, fl, family = _general_call(h, torch, I, n, 0, n, dev)
    assert family == GROUP
    with _auto(knobs) as h:
        v0, _, fl0, family = _general_call(h, torch, I, n, 0, n, dev, want_iters=False)
    assert family == GROUP
    u0, v0 = u0.T, v0.T
    _common(s, (u0,), it, fl, name)
    _spare_merged(s, (u0,), name)
    _common(s, (v0,), None, fl0, name + ", no iters")
    _spare_merged(s, (v0,), name + ", no iters")
    assert bits_equal(v0, u0)
    with _auto(knobs) as h:   # the plain entry
        w0, itw = h.solve_batch_general(*dev, inputs=I, want_iters=True)
        torch.cuda.synchronize()
        assert h.last_kernel_times()[2] == GROUP
        flw = h.last_flags
    _common(s, (w0.cpu().numpy().T,), itw.cpu().numpy(), flw, name + ", tpc_mpc_solve_batch_general")


@pytest.mark.parametrize("sharded", [True, False])
def test_general_form_presolve_in_a_wider_batch(torch_cuda, oracle, sharded):
    """The same block as columns [k0, k0+n) of a wider batch: the side rows keep the caller's leading dimension while the
    output base is shifted -- nothing outside the block's columns is written, inside it everything holds as above (the
    merge's evidence where the entry has a presolve: test_general_form_presolve)."""
    from trajectory_controller_amd.synth import general_inputs
    torch = torch_cuda
    name, I = "general_I2", 2
    s = _case(oracle, name)
    _route(torch, s, fits=True)
    g, knobs = _inputs(name)
    n, k0 = s.n, 130
    n_full = n + 700
    pad = general_inputs(40, n_full, I=I, first=99)   # valid instances around the block: none of them may be solved
    arrays = []
    for k in pc.GEN_NAMES:
        full = np.array(pad[k].reshape(n_full, -1).T, order="C", copy=True)
        full[:, k0:k0 + n] = g[k].reshape(n, -1).T
        arrays.append(torch.from_numpy(full).to("cuda:0"))
    with _auto(knobs) as h:
        u0, it, fl, family = _general_call(h, torch, I, n_full, k0, n, arrays, sharded=sharded)
    assert family == GROUP
    outside = np.ones(n_full, dtype=bool)
    outside[k0:k0 + n] = False
    assert np.all(u0[:, outside] == SENT) and np.all(it[outside] == -5)
    got = np.ascontiguousarray(u0[:, k0:k0 + n].T)
    _common(s, (got,), it[k0:k0 + n], fl, name + " in a wider batch")
    if sharded:
        _spare_merged(s, (got,), name + " in a wider batch")


def _mixed_check(bins, f, r, it, label):
    """the common assertions per bin; returns whether anything capped"""
    any_capped = False
    for H, (idx, b) in bins.items():
        _common(b, (f[idx], r[idx]), None if it is None else it[idx], None, f"{label}, N = {H}")
        any_capped = any_capped or bool(b.capped.any())
    return any_capped


@pytest.mark.parametrize("want_iters", [True, False])
@pytest.mark.parametrize("name", ["mixed", "mixed_default"])
def test_mixed_entry_under_auto(torch_cuda, oracle, name, want_iters):
    """The mixed-horizon entry: the N = 40 bin's presolve starts before the first bin and is finished behind the last,
    every other bin (and its own second pass) runs meanwhile on the share of the chip the presolve leaves."""
    from trajectory_controller_amd import FLAG_MAX_ITER
    torch = torch_cuda
    bins = _case(oracle, name)
    (hz, v, dy, dphi), knobs = _inputs(name)
    _route(torch, bins[40][1], fits=True)
    x = _dev(torch, v, dy, dphi)

    def call(h, hz):
        res = h.solve_batch_compact_mixed(hz, *x, want_iters=want_iters)
        torch.cuda.synchronize()
        f, r = _np(*res[:2])
        return f, r, (res[2].cpu().numpy() if want_iters else None), h.last_flags

    with _auto(knobs, H=20) as h:
        f, r, it, fl = call(h, hz)
        # the same instances with the sizes of the N = 20 and N = 40 bins swapped, on the same handle
        key = name + "/swapped"
        if key not in _solved:
            hz2 = pc.mixed_inputs(pc.MIXED_BINS_SWAPPED)[0]
            _solved[key] = (hz2, pc.solve_mixed(oracle, hz2, v, dy, dphi, knobs))
        hz2, bins2 = _solved[key]
        f2, r2, it2, fl2 = call(h, hz2)
    assert _mixed_check(bins, f, r, it, name) and fl & FLAG_MAX_ITER
    idx, b40 = bins[40]
    _spare_merged(b40, (f[idx], r[idx]), name + ", N = 40")
    assert _mixed_check(bins2, f2, r2, it2, key) == bool(fl2 & FLAG_MAX_ITER)
    # a family demanded explicitly: the bins run concurrently on child handles; LANE is dlib's arithmetic throughout
    with _auto(knobs, H=20, algo="lane") as h:
        fL, rL, itL, flL = call(h, hz)
    assert flL & FLAG_MAX_ITER
    for H, (idx, b) in bins.items():
        assert bits_equal(fL[idx], b.out[0]) and bits_equal(rL[idx], b.out[1]), H
        assert itL is None or np.array_equal(itL[idx], b.oit), H


def test_two_handles_presolving_at_once(torch_cuda, oracle):
    """Two handles, each with a presolve in flight, on two streams: nothing of the choreography (side stream, events,
    scratch, the queue's words) is shared between handles -- each batch equals its own single-handle result."""
    from trajectory_controller_amd.synth import compact_inputs
    torch = torch_cuda
    s = _case(oracle, "fits")
    _route(torch, s, fits=True)
    xa, knobs = _inputs("fits")
    xa, xb = _dev(torch, *xa), _dev(torch, *compact_inputs(40, s.n, first=90000))
    with _auto(knobs) as ha, _auto(knobs) as hb:
        fa, ra, ita, fla = _compact_on(torch, ha, xa)
        fb, rb, itb, _ = _compact_on(torch, hb, xb)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            ga = ha.solve_batch_compact(*xa, want_iters=True, want_flags=False)   # (no flags: the call does not wait)
        with torch.cuda.stream(sb):
            gb = hb.solve_batch_compact(*xb, want_iters=True, want_flags=False)
        torch.cuda.synchronize()
        ga, gb = _np(*ga), _np(*gb)
    _common(s, (fa, ra), ita, fla, "fits")
    _spare_merged(s, (fa, ra), "fits")
    for got, want in ((ga, (fa, ra, ita)), (gb, (fb, rb, itb))):
        assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
