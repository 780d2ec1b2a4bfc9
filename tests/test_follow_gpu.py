"""`-m gpu`: the raw-trajectory entries, tpc_mpc_follow_batch and tpc_mpc_follow_batch_horizon (csrc/mpc_follow.hip and
their staging in csrc/tpc_mpc_api.cpp), built on composition so that no solver family's tolerance enters:

  geometry     the targets, target_speed and target_distance equal tests/model/follow_ref.py bit for bit (signed zeros
               included) on the edge batches and the random one; phi is within 1e-15 of glibc's atan2 (the bound the
               first horizon test uses for device against glibc).  The horizon entry's reference is H independent walks.
  composition  each entry equals, bit for bit, the solve entry that is tested elsewhere fed the entry's own device
               targets -- in every family, at every horizon, with AUTO's cap guarantee on and off.
  glue         shards (ld > n, shifted base), the max_points clamp, streams, argument errors and flags through the C entry.

tests/test_follow_host.py holds the reference to the module shim on the CPU and asserts that the edge batches do sit on
their edges."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal, bits_equal32
from tests.model import follow_ref as fr

pytestmark = pytest.mark.gpu

GROUP_BUILT = [(10, 2), (10, 4), (20, 2), (20, 4), (20, 8), (40, 4), (40, 8)]   # as tests/test_groupg_gpu.py selects them
GEOMETRY_H = (1, 4, 7, 10, 20, 40, 64)
PHI_TOL = 1e-15
SENT = 777.25
TRAJ = ("px", "py", "dx", "dy", "vel")
T_STEP, WHEELBASE = 0.1, 0.21                                                   # tpc_mpc_default_params


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _solver(H, family="lane", **kw):
    from trajectory_controller_amd import MpcSolver, capi
    name, arg = family if isinstance(family, tuple) else (family, None)
    s = MpcSolver(horizon=H, device=0, dtype="f64", algo=name, **kw)
    if name == "group":
        s.set_option(capi.OPT_GROUP_LANES, arg)
    return s


def _fid(p):
    fam, H = p
    return (fam if isinstance(fam, str) else f"{fam[0]}-g{fam[1]}") + f"-H{H}"


def _g(torch, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the cached batches are read-only)


def _dev(torch, b):
    return [_g(torch, b[k]) for k in fr.FIELDS]


def _table(torch, name):
    tab = fr.TABLES[name]
    return (None, (None, None)) if tab is None else ((_g(torch, tab[0]), _g(torch, tab[1])), tab)


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


_cache = {}


def _batch(name, n):
    """The batches are deterministic: built once per module run and left unchanged."""
    if (name, n) not in _cache:
        b = (fr.random_batch(n, 24, 5) if name == "random" else fr.mixed_batch() if name == "mixed" else
             fr.capped_batch(n) if name == "capped" else fr.EDGE_BUILDERS[name](n))
        for a in b.values():
            if a is not None:
                a.setflags(write=False)
        _cache[name, n] = b
    return _cache[name, n]


# ---------------------------------------------------------------------------------------------
# 1. geometry, exact

def _check_geometry(H, b, spacing, tab, ts, td, tg=None, max_points=None):
    traj = [b[k] for k in TRAJ]
    if tg is None:
        one = fr.traj_points(*traj, b["count"], b["look"], max_points)
    else:
        if spacing is None:
            spacing = fr.default_spacing(fr.lut_batch(b["carv"], *tab), T_STEP)
        steps = fr.horizon_batch(*traj, b["count"], b["look"], spacing, H, max_points)
        one = steps[0]
        want = fr.targets_of(steps)
        assert tg.shape == want.shape
        assert bits_equal(tg[0::2], want[0::2]), "y targets"
        assert np.abs(tg[1::2] - want[1::2]).max() <= PHI_TOL, "phi targets"
    assert bits_equal32(ts, one["ovel"]), "target_speed"
    assert bits_equal32(td, one["dist"]), "target_distance"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
@pytest.mark.parametrize("name", list(fr.EDGE_BUILDERS) + ["random"])
def test_geometry_is_the_reference_bit_for_bit(torch_cuda, name, n):
    from trajectory_controller_amd import FLAG_NONFINITE
    torch = torch_cuda
    b = _batch(name, n)
    dev = _dev(torch, b)
    tables = list(fr.TABLES) if name == "speed" else ["none", "four"] if name == "random" else ["none"]
    # the batch's own spacing; the default too where the speed (the table) is what the batch is about
    spacings = [None] if name in ("speed", "random") else [b["spacing"], None] if name == "spacing" else [b["spacing"]]
    with _solver(10, "auto") as s:                  # the single point depends neither on the horizon nor on the table
        f, r, ts, td = s.follow_batch(*dev, lookup=_table(torch, tables[-1])[0])
        assert s.last_flags & FLAG_NONFINITE == 0
        _check_geometry(10, b, None, None, *_np(ts, td))
    for H in GEOMETRY_H:
        with _solver(H, "auto") as s:
            for tname in tables:
                lookup, tab = _table(torch, tname)
                for sp in spacings:
                    f, r, ts, td, tg = s.follow_batch_horizon(*dev, step_spacing=_g(torch, sp), lookup=lookup, want_targets=True)
                    assert s.last_flags & FLAG_NONFINITE == 0
                    _check_geometry(H, b, sp, tab, *_np(ts, td, tg))


# ---------------------------------------------------------------------------------------------
# 2. composition, bit for bit, every family

COMPACT_FAMILIES = ([(a, H) for a in ("lane", "lane_fma", "wave", "auto") for H in (4, 10, 20, 40)] +
                    [(("group", G), H) for H, G in GROUP_BUILT] + [("auto", 7), ("lane", 7)])
GENERAL_FAMILIES = ([(a, H) for a in ("lane", "wave", "auto") for H in (4, 10, 20, 40)] +
                    [("lane_fma", H) for H in (4, 10, 20)] + [(("group", G), H) for H, G in GROUP_BUILT] +
                    [("auto", 7), ("lane", 7)])


def _crossing(ts, *arrays):
    out = [a.copy() for a in arrays]
    for a in out:
        a[ts < np.float32(0.5)] = 0.0
    return out


def _compose_compact(torch, s, b, dev, lookup, tab, **over):
    """What follow_batch must return, from the tested entries: the device's own (y, phi) of the look-ahead point (the
    horizon entry with spacing 0), the reference speed, solve_batch_compact, the crossing rule in numpy."""
    n = len(b["count"])
    zero = torch.zeros(n, dtype=torch.float32, device="cuda")
    _, _, ts, _, tg = s.follow_batch_horizon(*dev, step_spacing=zero, lookup=lookup, want_targets=True, **over)
    v = _g(torch, fr.lut_batch(b["carv"], *tab).astype(np.float64))
    f, r, it = s.solve_batch_compact(v, tg[0].contiguous(), tg[1].contiguous(), want_iters=True, **over)
    flags = s.last_flags
    ts, f, r, it, tg = _np(ts, f, r, it, tg)
    f, r = _crossing(ts, f, r)
    return f, r, it, flags, v.cpu().numpy(), tg


def _general_arrays(torch, s, b, tab):
    n = len(b["count"])
    p = s.params
    v = fr.lut_batch(b["carv"], *tab).astype(np.float64)
    A, B = fr.compact_model(v, p.step_size, p.wheelbase)
    rows = lambda a, c: np.ascontiguousarray(np.tile(np.asarray([a, c], dtype=np.float64)[:, None], (1, n)))
    z2 = np.zeros((2, n))
    arrays = [A, B, z2, rows(p.weight_y, p.weight_phi), rows(p.weight_steering_front, p.weight_steering_rear),
              rows(p.lower[0], p.lower[1]), rows(p.upper[0], p.upper[1]), z2]
    return arrays, [_g(torch, a) for a in arrays]


@pytest.mark.parametrize("fam_h", COMPACT_FAMILIES, ids=_fid)
def test_follow_batch_is_the_compact_solve_of_its_own_targets(torch_cuda, oracle, fam_h):
    torch = torch_cuda
    family, H = fam_h
    b = _batch("mixed", 0)
    dev = _dev(torch, b)
    for tname in ("none", "four"):
        lookup, tab = _table(torch, tname)
        with _solver(H, family) as s:
            f, r, ts, td, it = s.follow_batch(*dev, lookup=lookup, want_iters=True)
            flags = s.last_flags
            f, r, ts, it = _np(f, r, ts, it)
            wf, wr, wit, wflags, v, tg = _compose_compact(torch, s, b, dev, lookup, tab)
        assert np.array_equal(it, wit) and flags == wflags, (family, H, tname)
        assert bits_equal(f, wf) and bits_equal(r, wr), (family, H, tname)
        assert np.any(f != 0) and np.any(ts < np.float32(0.5))
        if family == "lane" and H in (4, 20):          # and LANE is dlib's arithmetic: the oracle's bits
            of, orr, oit = oracle.solve_compact(H, v, tg[0], tg[1], nthreads=8)
            of, orr = _crossing(ts, of, orr)
            assert np.array_equal(it, oit) and bits_equal(f, of) and bits_equal(r, orr), (H, tname)


@pytest.mark.parametrize("fam_h", GENERAL_FAMILIES, ids=_fid)
def test_follow_batch_horizon_is_the_general_solve_of_its_own_targets(torch_cuda, oracle, fam_h):
    torch = torch_cuda
    family, H = fam_h
    b = _batch("mixed", 0)
    n = len(b["count"])
    dev = _dev(torch, b)
    for tname, sp in (("none", b["spacing"]), ("four", None)):
        lookup, tab = _table(torch, tname)
        with _solver(H, family) as s:
            f, r, ts, td, tg, it = s.follow_batch_horizon(*dev, step_spacing=_g(torch, sp), lookup=lookup, want_targets=True,
                                                          want_iters=True)
            flags = s.last_flags
            host, gen = _general_arrays(torch, s, b, tab)
            u0, wit = s.solve_batch_general(*gen, tg, inputs=2, want_iters=True)
            wflags = s.last_flags
        f, r, ts, it, u0, wit, tg = _np(f, r, ts, it, u0, wit, tg)
        wf, wr = _crossing(ts, u0[0], u0[1])
        assert np.array_equal(it, wit) and flags == wflags, (family, H, tname)
        assert bits_equal(f, wf) and bits_equal(r, wr), (family, H, tname)
        assert np.any(f != 0)
        if family == "lane" and H in (4, 20):
            ou0, _, oit = oracle.solve_general(2, H, *[a.T for a in host], tg.T.reshape(n, H, 2), nthreads=8)
            of, orr = _crossing(ts, ou0[:, 0], ou0[:, 1])
            assert np.array_equal(it, oit) and bits_equal(f, of) and bits_equal(r, orr), (H, tname)


def test_wave_at_a_horizon_it_does_not_have_is_refused(torch_cuda):
    from trajectory_controller_amd import capi
    torch = torch_cuda
    b = _batch("random", 65)
    dev = _dev(torch, b)
    with _solver(7, "wave") as s:
        for call in (s.follow_batch, s.follow_batch_horizon):
            with pytest.raises(capi.TpcMpcError) as e:
                call(*dev)
            assert e.value.status == 4                          # TPC_MPC_ERR_BAD_HORIZON
        # ... and the handle is still good: the same request under LANE, against a fresh handle
        got = _np(*s.follow_batch_horizon(*dev, want_targets=True, want_iters=True, algo=capi.ALGO_LANE))
    with _solver(7, "lane") as s:
        want = _np(*s.follow_batch_horizon(*dev, want_targets=True, want_iters=True))
    assert all(bits_equal(a, c) if a.dtype == np.float64 else np.array_equal(a, c, equal_nan=True) for a, c in zip(got, want))


# ---------------------------------------------------------------------------------------------
# 3. AUTO's guarantee inside the follow entries

CAP = 50


@pytest.mark.parametrize("fast", [False, True], ids=["guarantee", "fast_capped"])
def test_auto_cap_resolve_inside_the_follow_entries(torch_cuda, oracle, fast):
    """H = 40 and max_iter = 50: AUTO's tolerance family leaves a good share of the batch on the cap, and the bit-exact
    re-solve of those (or, with TPC_MPC_PARAM_FAST_CAPPED, its absence) must be the composed solve entry's -- with the
    caller's iteration counts and without (the follow entries then take the handle's own buffer)."""
    from trajectory_controller_amd import FLAG_MAX_ITER, capi
    torch = torch_cuda
    H, n = 40, 1230
    b = _batch("capped", n)
    dev = _dev(torch, b)
    over = dict(max_iter=CAP, options=capi.PARAM_FAST_CAPPED if fast else 0)
    with _solver(H, "auto") as s:
        # follow_batch
        f, r, ts, td, it = s.follow_batch(*dev, want_iters=True, **over)
        flags = s.last_flags
        f2, r2, _, _ = s.follow_batch(*dev, want_iters=False, **over)
        f, r, it, f2, r2 = _np(f, r, it, f2, r2)
        wf, wr, wit, wflags, v, tg = _compose_compact(torch, s, b, dev, None, (None, None), **over)
        _, _, oit = oracle.solve_compact(H, v, tg[0], tg[1], max_iter=CAP, nthreads=8)
        assert (oit >= CAP).mean() >= 0.10 and (oit < CAP).mean() >= 0.10
        assert np.array_equal(it, wit) and flags == wflags and flags & FLAG_MAX_ITER
        assert bits_equal(f, wf) and bits_equal(r, wr)
        assert bits_equal(f2, wf) and bits_equal(r2, wr)
        # follow_batch_horizon
        sp = _g(torch, b["spacing"])
        f, r, ts, td, tg, it = s.follow_batch_horizon(*dev, step_spacing=sp, want_targets=True, want_iters=True, **over)
        flags = s.last_flags
        f2, r2, _, _ = s.follow_batch_horizon(*dev, step_spacing=sp, **over)
        host, gen = _general_arrays(torch, s, b, (None, None))
        u0, wit = s.solve_batch_general(*gen, tg, inputs=2, want_iters=True, **over)
        wflags = s.last_flags
        f, r, ts, it, f2, r2, u0, wit, tg = _np(f, r, ts, it, f2, r2, u0, wit, tg)
        _, _, oit = oracle.solve_general(2, H, *[a.T for a in host], tg.T.reshape(n, H, 2), max_iter=CAP, nthreads=8)
        assert (oit >= CAP).mean() >= 0.10 and (oit < CAP).mean() >= 0.10
        wf, wr = _crossing(ts, u0[0], u0[1])
        assert np.array_equal(it, wit) and flags == wflags and flags & FLAG_MAX_ITER
        assert bits_equal(f, wf) and bits_equal(r, wr)
        assert bits_equal(f2, wf) and bits_equal(r2, wr)


# ---------------------------------------------------------------------------------------------
# 4. the C entry: shards, clamps, streams, arguments, flags

class _Out:
    """Output buffers of one call, over-allocated and pre-filled, the call's part starting `off` elements in."""

    def __init__(self, torch, n, H, off=11, extra=50):
        self.n, self.H, self.off = n, H, off
        mk = lambda dt, fill, m: torch.full((m,), fill, dtype=dt, device="cuda")
        self.front, self.rear = mk(torch.float64, SENT, n + extra), mk(torch.float64, SENT, n + extra)
        self.ts, self.td = mk(torch.float32, SENT, n + extra), mk(torch.float32, SENT, n + extra)
        self.iters = mk(torch.int32, -5, n + extra)
        self.targets = mk(torch.float64, SENT, 2 * H * n + extra)

    def ptr(self, t):
        return t.data_ptr() + self.off * t.element_size()

    def results(self, horizon_entry):
        sl = slice(self.off, self.off + self.n)
        out = [a.cpu().numpy() for a in (self.front, self.rear, self.ts, self.td, self.iters)]
        for a in out:                                           # nothing outside the call's n elements was written
            outside = np.delete(a, sl)
            assert np.all(outside == (-5 if a.dtype == np.int32 else SENT))
        res = [a[sl] for a in out]
        tg = self.targets.cpu().numpy()
        if horizon_entry:
            assert np.all(tg[2 * self.H * self.n:] == SENT)
            res.append(tg[:2 * self.H * self.n].reshape(2 * self.H, self.n))    # leading dimension n, as the header says
        else:
            assert np.all(tg == SENT)
        return res


def _raw(s, horizon_entry, tr, out, spacing=None, lookup=(None, None, 0), flags=True, stream=None, params=None, iters=True,
         **null):
    """The C entry itself.  `null`: names of output pointers to pass as NULL.  Returns (status, flags)."""
    fl = C.c_uint32(0xDEAD)
    p = params if params is not None else s.params
    ptr = lambda name: None if null.get(name) else out.ptr(getattr(out, name))
    common = (ptr("front"), ptr("rear"), ptr("ts"), ptr("td"))
    ip = out.ptr(out.iters) if iters else None
    trp = None if tr is None else C.byref(tr)
    if horizon_entry:
        rc = s._lib.tpc_mpc_follow_batch_horizon(s._h, C.byref(p), trp, spacing, *lookup, *common, out.targets.data_ptr(), ip,
                                                 C.byref(fl) if flags else None, stream)
    else:
        rc = s._lib.tpc_mpc_follow_batch(s._h, C.byref(p), trp, *lookup, *common, ip, C.byref(fl) if flags else None, stream)
    return rc, fl.value


def _trajectories(dev, n, ld, max_points, k0=0):
    from trajectory_controller_amd import capi
    at = lambda t: t.data_ptr() + k0 * t.element_size()
    return capi.Trajectories(n=n, ld=ld, max_points=max_points, pos_x=at(dev[0]), pos_y=at(dev[1]), dir_x=at(dev[2]),
                             dir_y=at(dev[3]), velocity=at(dev[4]), count=at(dev[5]), car_velocity=at(dev[6]),
                             look_ahead=at(dev[7]))


SHARD = dict(H=10, n=333, P=24, max_points=16, k0=19, pad=37)


def _shard_case():
    """The shard test's batch: random polylines whose look-aheads reach past the arc length of row max_points - 1 in a
    good share of the columns, inside arrays `pad` wider than n.  Every column outside [k0, k0 + n) and every row at or
    past min(count, max_points) holds NaN.  Returns (b, clamped counts, the wide arrays, the wide spacing)."""
    n, P, max_points, k0 = SHARD["n"], SHARD["P"], SHARD["max_points"], SHARD["k0"]
    ld = n + SHARD["pad"]
    b = fr.random_batch(n, P, 21)
    rng = np.random.default_rng(2)
    b["look"] = rng.uniform(0.2, 4.0, size=n).astype(np.float32)
    clamped = np.minimum(b["count"], max_points)
    wide = {}
    for k in TRAJ:
        a = np.full((P, ld), np.nan, dtype=np.float32)
        a[:, k0:k0 + n] = np.where(np.arange(P)[:, None] < clamped[None, :], b[k], np.float32(np.nan))
        wide[k] = a
    for k, fill in (("count", 2 ** 30), ("carv", np.nan), ("look", np.nan)):
        a = np.full(ld, fill, dtype=b[k].dtype)
        a[k0:k0 + n] = b[k]
        wide[k] = a
    spacing = np.full(ld, np.nan, dtype=np.float32)
    spacing[k0:k0 + n] = rng.uniform(-0.05, 0.3, size=n).astype(np.float32)
    return b, clamped, wide, spacing


def _differs(one, other, keys=("oy", "ovel", "dist")):
    return np.any([~((one[k].view(np.uint32) == other[k].view(np.uint32)) | (np.isnan(one[k]) & np.isnan(other[k])))
                   for k in keys], axis=0)


@pytest.mark.parametrize("horizon_entry", [False, True], ids=["follow_batch", "follow_batch_horizon"])
def test_shard_of_a_wider_batch_and_the_max_points_clamp(torch_cuda, horizon_entry):
    """Columns [19, 19 + n) of arrays 37 wider than n, every column outside them NaN, every row at or past
    min(count, max_points) NaN, count > max_points in a good share of the columns: the bits of the contiguous call on
    the clamped counts, nothing written past n, flags 0.  From the reference first: a walk without the clamp (it reads
    the NaN rows, or takes another last point) differs from the clamped one on at least 10 % of the columns for the
    single-point entry, and so for step 0 of the horizon entry -- the clamp decides the result there."""
    torch = torch_cuda
    H, n, P, max_points, k0 = (SHARD[k] for k in ("H", "n", "P", "max_points", "k0"))
    ld = n + SHARD["pad"]
    b, clamped, wide, spacing = _shard_case()
    shard = [wide[k][:, k0:k0 + n] for k in TRAJ]
    with_clamp = fr.traj_points(*shard, b["count"], b["look"], max_points)
    assert _differs(with_clamp, fr.traj_points(*shard, b["count"], b["look"])).mean() >= 0.10
    assert not _differs(with_clamp, fr.traj_points(*[b[k] for k in TRAJ], clamped, b["look"])).any()
    lut_x, lut_y = fr.TABLES["four"]
    dl = (_g(torch, lut_x), _g(torch, lut_y))
    with _solver(H, "lane") as s:
        contiguous = [_g(torch, b[k]) for k in TRAJ] + [_g(torch, clamped), _g(torch, b["carv"]), _g(torch, b["look"])]
        if horizon_entry:
            want = s.follow_batch_horizon(*contiguous, step_spacing=_g(torch, spacing[k0:k0 + n]), lookup=dl,
                                          want_targets=True, want_iters=True)
            want = [want[i] for i in (0, 1, 2, 3, 5, 4)]
        else:
            want = s.follow_batch(*contiguous, lookup=dl, want_iters=True)
        want = _np(*want)
        dev = [_g(torch, wide[k]) for k in fr.FIELDS]
        dsp = _g(torch, spacing)
        out = _Out(torch, n, H)
        rc, flags = _raw(s, horizon_entry, _trajectories(dev, n, ld, max_points, k0), out,
                         spacing=dsp.data_ptr() + 4 * k0, lookup=(dl[0].data_ptr(), dl[1].data_ptr(), len(lut_x)))
        torch.cuda.synchronize()
        assert rc == 0 and flags == 0, s._lib.tpc_mpc_last_error(s._h)
        got = out.results(horizon_entry)
    for a, c in zip(got, want):
        assert bits_equal(a, c, dtype=a.dtype) if a.dtype != np.int32 else np.array_equal(a, c)
    # and the reference, so that the contiguous call is not the only witness of the clamp
    _check_geometry(H, b, spacing[k0:k0 + n], (lut_x, lut_y), got[2], got[3], got[5] if horizon_entry else None,
                    max_points=max_points)


def test_side_stream_and_two_entries_back_to_back(torch_cuda):
    """The same call on a side stream with flags_out = NULL (asynchronous: the stream is synchronised afterwards), then
    follow_batch and follow_batch_horizon back to back on one handle and one stream -- they share the handle's scratch,
    and each must return its own result."""
    torch = torch_cuda
    H, n = 10, 1230
    b = _batch("mixed", 0)
    dev = _dev(torch, b)
    sp = _g(torch, b["spacing"])
    tr = _trajectories(dev, n, n, b["px"].shape[0])
    with _solver(H, "auto") as s:
        want1 = _np(*s.follow_batch(*dev, want_iters=True))
        w = s.follow_batch_horizon(*dev, step_spacing=sp, want_targets=True, want_iters=True)
        want2 = _np(*[w[i] for i in (0, 1, 2, 3, 5, 4)])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        o1, o2 = _Out(torch, n, H), _Out(torch, n, H)
        torch.cuda.synchronize()
        st = C.c_void_p(side.cuda_stream)
        rc1, _ = _raw(s, False, tr, o1, flags=False, stream=st)
        rc2, _ = _raw(s, True, tr, o2, spacing=sp.data_ptr(), flags=False, stream=st)
        side.synchronize()
        assert rc1 == 0 and rc2 == 0
        for got, want in ((o1.results(False), want1), (o2.results(True), want2)):
            for a, c in zip(got, want):
                assert bits_equal(a, c, dtype=a.dtype) if a.dtype != np.int32 else np.array_equal(a, c)
        # the other order, on the default stream, with flags
        o1, o2 = _Out(torch, n, H), _Out(torch, n, H)
        rc2, fl2 = _raw(s, True, tr, o2, spacing=sp.data_ptr())
        rc1, fl1 = _raw(s, False, tr, o1)
        torch.cuda.synchronize()
        assert (rc1, rc2) == (0, 0)
        for got, want in ((o1.results(False), want1), (o2.results(True), want2)):
            for a, c in zip(got, want):
                assert bits_equal(a, c, dtype=a.dtype) if a.dtype != np.int32 else np.array_equal(a, c)
    assert not bits_equal(want1[0], want2[0])                 # (the two entries do answer differently)


@pytest.mark.parametrize("horizon_entry", [False, True], ids=["follow_batch", "follow_batch_horizon"])
def test_arguments(torch_cuda, horizon_entry):
    from trajectory_controller_amd import MpcSolver, capi
    torch = torch_cuda
    BAD_ARG, NO_DEVICE = 1, 6
    H, n = 10, 65
    b = _batch("random", n)
    dev = _dev(torch, b)
    P = b["px"].shape[0]
    out = _Out(torch, n, H)
    with _solver(H, "lane") as s:
        # n = 0: OK, flags 0, nothing read (every pointer may be null) or written
        empty = capi.Trajectories(n=0, ld=0, max_points=0)
        assert _raw(s, horizon_entry, empty, out) == (0, 0)
        bad = [_trajectories(dev, n, n - 1, P), _trajectories(dev, n, n, -1), _trajectories(dev, -1, n, P)]
        for name in ("pos_x", "pos_y", "dir_x", "dir_y", "velocity", "count", "car_velocity", "look_ahead"):
            tr = _trajectories(dev, n, n, P)
            setattr(tr, name, None)
            bad.append(tr)
        for tr in bad + [None]:
            assert _raw(s, horizon_entry, tr, out)[0] == BAD_ARG
        good = _trajectories(dev, n, n, P)
        assert _raw(s, horizon_entry, good, out, lookup=(None, None, -1))[0] == BAD_ARG
        assert _raw(s, horizon_entry, good, out, lookup=(None, None, 2))[0] == BAD_ARG          # a table without its arrays
        f32 = capi.Params.from_buffer_copy(s.params)
        f32.dtype = capi.F32
        assert _raw(s, horizon_entry, good, out, params=f32)[0] == BAD_ARG
        for name in ("front", "rear", "ts", "td"):
            assert _raw(s, horizon_entry, good, out, **{name: True})[0] == BAD_ARG
        torch.cuda.synchronize()
        for a in out.results(False):                             # none of the refused calls wrote anything: not outside
            assert np.all(a == (-5 if a.dtype == np.int32 else SENT))       # the call's n elements, and not inside them
        assert _raw(s, horizon_entry, good, out) == (0, 0)       # and the handle still serves
        torch.cuda.synchronize()
    with MpcSolver(horizon=H, device=None) as hst:
        assert _raw(hst, horizon_entry, good, out)[0] == NO_DEVICE


@pytest.mark.parametrize("horizon_entry", [False, True], ids=["follow_batch", "follow_batch_horizon"])
def test_non_finite_inputs_and_the_flag(torch_cuda, horizon_entry):
    """A NaN car_velocity (no lookup table: the table's search would answer a NaN with its last value, as the shim's
    does) and a NaN in the direction of the point that is read make that instance's solve non-finite: FLAG_NONFINITE,
    steering at the start point 0, every other instance's bits untouched.  A NaN target_speed is not an input of the
    solve and `NaN < 0.5` is false, as in the shim: the steering stays."""
    from trajectory_controller_amd import FLAG_NONFINITE
    torch = torch_cuda
    H, n = 10, 130
    clean = {k: a.copy() for k, a in fr.random_batch(n, 24, 33).items() if a is not None}
    clean["vel"][:] = np.maximum(clean["vel"], np.float32(0.6))          # no instance is zeroed by the crossing rule
    clean["count"][:] = np.maximum(clean["count"], 3)
    one = fr.traj_points(*[clean[k] for k in TRAJ], clean["count"], clean["look"])
    k_v, k_dir, k_ts = 7, 64, 129
    dirty = {k: a.copy() for k, a in clean.items()}
    dirty["carv"][k_v] = np.nan
    row = lambda k: one["seg"][k] if one["seg"][k] >= 1 else clean["count"][k] - 1       # the point instance k reads
    dirty["dy"][row(k_dir), k_dir] = np.nan
    dirty["vel"][row(k_ts), k_ts] = np.nan
    zero = torch.zeros(n, dtype=torch.float32, device="cuda")
    call = lambda s, b: ((s.follow_batch_horizon(*_dev(torch, b), step_spacing=zero, want_iters=True) if horizon_entry else
                          s.follow_batch(*_dev(torch, b), want_iters=True)), s.last_flags)
    with _solver(H, "lane") as s:
        (wf, wr, wts, wtd, wit), wflags = call(s, clean)
        (f, r, ts, td, it), flags = call(s, dirty)
    wf, wr, wts, wit, f, r, ts, it = _np(wf, wr, wts, wit, f, r, ts, it)
    assert wflags & FLAG_NONFINITE == 0 and flags & FLAG_NONFINITE
    good = np.ones(n, dtype=bool)
    good[[k_v, k_dir]] = False
    assert bits_equal(f[good], wf[good]) and bits_equal(r[good], wr[good]) and np.array_equal(it[good], wit[good])
    assert np.all(f[~good] == 0) and np.all(r[~good] == 0) and np.all(it[~good] == 0)
    assert np.isnan(ts[k_ts]) and wf[k_ts] != 0 and f[k_ts] == wf[k_ts] and r[k_ts] == wr[k_ts]
    assert bits_equal32(np.delete(ts, k_ts), np.delete(wts, k_ts))
