"""tests/model/rollout_device_paths.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What tests/test_rollout_device_paths_host.py and _gpu.py share: the batches, the C entries of the closed loops and of
their derivatives called through capi on arrays that are wider than the batch, and an independent reference of every
entry.

Memory.  A `Mem` hands out the arrays of one call: HOST numpy or DEVICE torch arrays of `ld = n + pad` columns with
the batch at column `off` (the disturbance's arrays have `ld_d = n + pad_d`); inputs are padded with NaN, outputs and
in/outs are filled with a sentinel.  `Mem(n)` is the packed HOST layout (ld = n) the references are computed in.

References, each [rows, n], computed once per (case, entry, which optional INPUTS were given) with every output:
  newton, FALLBACK_NONE; both backwards; every forward   the same C entry on a host-only handle
  rollout, rollout_record, rollout_polished               `solve_loop`: the oracle's operator() carrying controls and v,
      (and the plant's RECORD / POLISHED loops)           polish_batch_general on a host-only handle, the plant's line
                                                          and the target shift in numpy (mpc_rollout_polish_ref.replay
                                                          with the controller state in and out, a plant and a
                                                          disturbance).  The LANE kernels are dlib's bits
                                                          (tests/test_parity_gpu.py), so the device handle asks for LANE.
  newton, FALLBACK_SOLVE                                  the polished loop's columns where the FALLBACK_NONE pass has
                                                          first_unverified < steps, the FALLBACK_NONE bits elsewhere
                                                          (v out: the polished loop's v there, the sequence elsewhere)
"""
from __future__ import annotations

import ctypes as C
import functools
import types

import numpy as np

from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.test_rollout_plant_host import make_plant
from trajectory_controller_amd import MpcSolver, capi

TOL, ROUNDS = 1e-9, 8
OFF, PAD, PAD_D = 5, 13, 29            # the batch at column 5 of ld = n + 13 columns, ld_d = n + 29
SENTINEL, ISENTINEL = 12345.0, -7
SHAPES = [(2, 10, 4, 130), (1, 20, 3, 130), (2, 4, 3, 1)]     # (I, H, S, n): three wavefronts, two live lanes in the last
IO_KEYS = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets")
INT_ROWS = ("iters", "status", "first")
LOOPS = dict(record=capi.LOOP_RECORD, polished=capi.LOOP_POLISHED, newton=capi.LOOP_NEWTON)
MODES = (None, "abc", "d", "both")     # None: the parent entry; else tpc_mpc_rollout_plant with the plant's arrays / a disturbance

# the optional arrays of each loop ("c", "v": io->controls_inout, v_inout; "nlt": new_last_targets)
LOOP_OPTIONAL = dict(
    rollout=("states", "iters", "c", "v", "nlt"),
    record=("states", "iters", "c", "v", "nlt"),      # sequences_out is required
    polished=("states", "iters", "sequences", "status", "rin", "rout", "c", "v", "nlt"),
    newton=("states", "iters", "sequences", "first", "status", "rin", "rout", "c", "v", "nlt"))
# the two layouts whose offsets depend on what was given: the HOST staging buffer of the loops, and the compact batch of
# the Newton loop's fallback ("ctrl" is always there, "dist" is the plant's disturbance: present in modes d and both)
STAGE_ORDER = ("sequences", "status", "rin", "rout", "dist")
FALLBACK_ORDER = ("nlt", "ctrl", "states", "sequences", "rin", "rout", "dist")


def loop_rows(cs):
    I, H, S = cs.I, cs.H, cs.S
    return dict(controls=S * I, states=2 * S, iters=S, sequences=S * H * I, first=1, status=S, rin=S, rout=S,
                c=H * I, v=H * I)


def subsets(kind, mode):
    """The optional-array subsets of one loop, each a frozenset of names, without repeats: only what is required,
    everything, each one missing alone, each one present alone, and for every adjacent pair (a, b) of the two layout
    orders "a missing, b present" -- with every other array of that order missing and every array outside it present,
    which is none of the earlier subsets."""
    opt = LOOP_OPTIONAL[kind]
    out = [frozenset(), frozenset(opt)]
    out += [frozenset(opt) - {k} for k in opt] + [frozenset({k}) for k in opt]
    has_d = mode in ("d", "both")
    for order in (STAGE_ORDER, tuple(k for k in FALLBACK_ORDER if k != "ctrl")):   # controls_out is always there
        for a, b in zip(order, order[1:]):
            if (b == "dist" and not has_d) or a not in opt or (b != "dist" and b not in opt):
                continue
            out.append(frozenset(k for k in opt if k not in order) | ({b} - {"dist"}))
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


# ---- batches ---------------------------------------------------------------------------------------------------------

def _finish_case(I, H, S, ins, nl, zero_c0=False):
    n = ins[0].shape[1]
    plant, dist = make_plant(ins, I, S)
    rng = np.random.default_rng(100 + 7 * H + I)
    lo, hi = np.tile(ins[5], (H, 1)), np.tile(ins[6], (H, 1))
    c0 = np.zeros((H * I, n)) if zero_c0 else np.clip(0.2 * rng.standard_normal((H * I, n)), lo, hi)
    v0 = np.clip(c0 + 0.05 * rng.standard_normal((H * I, n)), lo, hi)
    G_u, G_x = rng.standard_normal((S * I, n)), rng.standard_normal((2 * S, n))
    return types.SimpleNamespace(I=I, H=H, S=S, n=n, ins=[np.ascontiguousarray(a) for a in ins],
                                 nl=np.ascontiguousarray(nl), plant=plant, dist=dist, c0=np.ascontiguousarray(c0),
                                 v0=np.ascontiguousarray(v0), G_u=G_u, G_x=G_x, key=(I, H, S, n, zero_c0))


# mpc_rollout_dense.batch's seed per shape: H + I as tests/test_rollout_plant_gpu.py::_case, except where that gives a
# fallback set of exactly 64 (asserted in tests/test_rollout_device_paths_host.py)
SEEDS = {(1, 20, 3, 130): 22}     # seed 21: 64 of 130 fall back with new_last_targets alone


@functools.lru_cache(maxsize=None)
def case(I, H, S, n, seed=None):
    """tests/test_rollout_plant_gpu.py::_case (mpc_rollout_dense.batch, make_plant) plus a controller state to start
    from (c0 in the box, v0 near it) and the loss gradients of the backward"""
    seed = SEEDS.get((I, H, S, n), H + I) if seed is None else seed
    th, nlt = rd.batch(I, H, S, n, seed=seed, with_nlt=True)
    return _finish_case(I, H, S, [dense.soa(th[k], n) for k in rd.NAMES], dense.soa(nlt, n))


ONE = (2, 10, 4, 130)
ONE_AT = 77


@functools.lru_cache(maxsize=None)
def one_fallback_case():
    """A batch of 130 whose fallback set is exactly instance 77 (ldc = 64, one live lane): columns of case(*ONE) the
    FALLBACK_NONE pass verifies at every step in every mode, with and without new_last_targets, from a zero start
    (repeated to fill the batch: the instances are independent), and at 77 one it verifies in none of them."""
    I, H, S, n = ONE
    src = _finish_case(I, H, S, case(*ONE).ins, case(*ONE).nl, zero_c0=True)
    firsts = np.stack([ref_loop(src, "newton", mode, "none", frozenset({"nlt"} if nlt else ()))["first"][0]
                       for mode in MODES for nlt in (True, False)])
    good, bad = np.flatnonzero((firsts == S).all(axis=0)), np.flatnonzero((firsts < S).all(axis=0))
    assert good.size >= 8 and bad.size >= 1, (good.size, bad.size)
    cols = np.resize(good, n)
    cols[ONE_AT] = bad[0]
    cs = _finish_case(I, H, S, [a[:, cols] for a in src.ins], src.nl[:, cols], zero_c0=True)
    cs.plant, cs.dist = tuple(np.ascontiguousarray(a[:, cols]) for a in src.plant), np.ascontiguousarray(src.dist[:, cols])
    cs.v0, cs.key = np.ascontiguousarray(src.v0[:, cols]), cs.key + ("one",)
    return cs


# ---- memory ----------------------------------------------------------------------------------------------------------

class Buf:
    def __init__(self, mem, w):
        self.mem, self.host = mem, w
        mem.keep.append(self)   # a launch on a side stream may still read it when the call returns
        if mem.device:
            import torch
            if mem.stream is None:
                self.t = torch.from_numpy(w).cuda()
            else:   # filled on the side stream later (Mem.upload): NaN until then
                self.t = torch.full(w.shape, float("nan") if w.dtype.kind == "f" else -1,
                                    dtype=torch.from_numpy(w).dtype, device="cuda")
                mem.pending.append((self.t, torch.from_numpy(w).pin_memory()))
        self.ptr = (self.t.data_ptr() if mem.device else w.ctypes.data) + mem.off * w.itemsize

    def get(self):
        return self.t.cpu().numpy() if self.mem.device else self.host


class Mem:
    """the arrays of one call: [rows, ld] with the batch at column off, in HOST or DEVICE memory"""

    def __init__(self, n, device=False, pad=0, off=0, pad_d=0, stream=None):
        self.n, self.device, self.off, self.ld, self.ld_d, self.stream = n, device, off, n + pad, n + pad_d, stream
        self.kind, self.pending, self.keep = (capi.DEVICE if device else capi.HOST), [], []

    def put(self, a, ld=None, fill=np.nan):
        """an input (padding NaN) or an in/out (padding `fill`): a [..., n] -> [rows, ld]"""
        ld = self.ld if ld is None else ld
        w = np.full((int(np.prod(a.shape[:-1])), ld), fill, dtype=a.dtype)
        w[:, self.off:self.off + self.n] = a.reshape(-1, self.n)
        return Buf(self, w)

    def out(self, rows, ld=None, integer=False):
        ld = self.ld if ld is None else ld
        return Buf(self, np.full((rows, ld), ISENTINEL, np.int32) if integer else np.full((rows, ld), SENTINEL))

    def upload(self):
        """the side stream's part: some busywork, then the copies that produce the inputs"""
        import torch
        torch.cuda.current_stream().synchronize()   # the NaN fills are done; nothing is queued on the default stream
        with torch.cuda.stream(self.stream):
            a = torch.ones((1024, 1024), device="cuda")
            for _ in range(20):
                a = (a @ a) * 1e-3
            for t, src in self.pending:
                t.copy_(src, non_blocking=True)
        self.pending = []

    def stream_ptr(self):
        return None if self.stream is None else C.c_void_p(self.stream.cuda_stream)

    def sync(self):
        if self.device:
            import torch
            torch.cuda.synchronize() if self.stream is None else self.stream.synchronize()


def wide(n, device, stream=None):
    return Mem(n, device, PAD, OFF, PAD_D, stream)


def check(buf, want, name=""):
    """the batch's columns are the reference's bytes, every padding column still holds its sentinel"""
    m, g = buf.mem, buf.get()
    want = np.asarray(want).reshape(-1, m.n)
    got = np.ascontiguousarray(g[:, m.off:m.off + m.n])
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        cols = np.flatnonzero((got.view(np.uint8).reshape(got.shape[0], m.n, -1)
                               != want.view(np.uint8).reshape(got.shape[0], m.n, -1)).any(axis=(0, 2)))
        raise AssertionError(f"{name}: {cols.size} of {m.n} columns differ, first {cols[:8].tolist()}, "
                             f"{int(np.isnan(got.astype(np.float64)).sum())} NaN")
    pad = ISENTINEL if g.dtype == np.int32 else SENTINEL
    assert np.all(g[:, :m.off] == pad) and np.all(g[:, m.off + m.n:] == pad), name + ": padding"


def _check_all(out, ref, decoy):
    """every output against its reference and the decoy, all failures in one message"""
    bad = []
    for k, b in out.items():
        try:
            check(b, ref[k], k)
        except AssertionError as e:
            bad.append(str(e))
    if not untouched(decoy):
        bad.append("the decoy was written")
    assert not bad, "; ".join(bad)


def untouched(buf):
    g = buf.get()
    return bool(np.all(g == (ISENTINEL if g.dtype == np.int32 else SENTINEL)))


def _p(b):
    return None if b is None else b.ptr


def _io(cs, mem):
    return capi.GeneralIO(inputs=cs.I, n=cs.n, ld=mem.ld, **{k: mem.put(a).ptr for k, a in zip(IO_KEYS, cs.ins)})


def _plant(cs, mem, mode, with_dist=True, ld_d=None):
    ab = [mem.put(a) for a in cs.plant] if mode in ("abc", "both") else [None] * 3
    d = mem.put(cs.dist, ld=mem.ld_d) if with_dist and mode in ("d", "both") else None
    return capi.Plant(A=_p(ab[0]), B=_p(ab[1]), C=_p(ab[2]), disturbance=_p(d), ld_d=mem.ld_d if ld_d is None else ld_d)


# ---- the loops -------------------------------------------------------------------------------------------------------

def run_loop(lib, s, cs, mem, kind, mode, fallback, present, launch_only=False):
    """One closed-loop entry with the optional arrays `present`; an array that is not given is not allocated.  Returns
    (rc, flags, {name: Buf}, decoy): the decoy is one more sentinel-filled array of the largest output's size that the
    call is not given."""
    I, H, S = cs.I, cs.H, cs.S
    rows, present = loop_rows(cs), set(present)
    io = _io(cs, mem)
    names = {"controls"} | ({"sequences"} if kind == "record" else set()) | (present & set(rows))
    out = {k: (mem.put({"c": cs.c0, "v": cs.v0}[k], fill=SENTINEL) if k in ("c", "v") else
               mem.out(rows[k], integer=k in INT_ROWS)) for k in sorted(names)}
    io.controls_inout, io.v_inout = _p(out.get("c")), _p(out.get("v"))
    nl = mem.put(cs.nl) if "nlt" in present else None
    decoy = mem.out(rows["sequences"])
    q = capi.Polish(tol=TOL, max_rounds=ROUNDS, reserved=0, status=_p(out.get("status")),
                    residual_in=_p(out.get("rin")), residual_out=_p(out.get("rout")))
    o = lambda k: _p(out.get(k))
    fb = capi.NEWTON_FALLBACK_SOLVE if fallback == "solve" else capi.NEWTON_FALLBACK_NONE
    flags, p, st = C.c_uint32(99), s._params(), mem.stream_ptr()
    fl = None if launch_only else C.byref(flags)   # asking for the flags waits for the stream
    pl = _plant(cs, mem, mode) if mode is not None else None
    if mem.pending:
        mem.upload()
    if mode is not None:
        rc = lib.tpc_mpc_rollout_plant(s._h, C.byref(p), C.byref(io), C.byref(pl), LOOPS[kind], S, _p(nl), C.byref(q),
                                       fb, o("controls"), o("states"), o("iters"), o("sequences"), o("first"),
                                       fl, mem.kind, st)
    elif kind == "rollout":
        rc = lib.tpc_mpc_rollout(s._h, C.byref(p), C.byref(io), S, _p(nl), o("controls"), o("states"), o("iters"),
                                 fl, mem.kind, st)
    elif kind == "record":
        rc = lib.tpc_mpc_rollout_record(s._h, C.byref(p), C.byref(io), S, _p(nl), o("controls"), o("states"),
                                        o("iters"), o("sequences"), fl, mem.kind, st)
    elif kind == "polished":
        rc = lib.tpc_mpc_rollout_polished(s._h, C.byref(p), C.byref(io), S, _p(nl), C.byref(q), o("controls"),
                                          o("states"), o("iters"), o("sequences"), fl, mem.kind, st)
    else:
        rc = lib.tpc_mpc_rollout_newton(s._h, C.byref(p), C.byref(io), S, _p(nl), C.byref(q), fb, o("controls"),
                                        o("states"), o("iters"), o("sequences"), o("first"), fl, mem.kind,
                                        st)
    if not launch_only:
        mem.sync()
    return rc, (None if launch_only else flags.value), out, decoy


def given_inputs(present):
    """what of a subset changes the numbers: the optional inputs"""
    return frozenset(present) & {"c", "v", "nlt"}


def solve_loop(cs, polished, mode, given):
    """The solve-based loops on the CPU (see the module's docstring): {name: [rows, n]}"""
    from oracle.bindings import Oracle
    o = Oracle()
    I, H, S, n = cs.I, cs.H, cs.S, cs.n
    aos = lambda a: np.ascontiguousarray(a.T)
    model = [aos(a) for a in cs.ins[:7]]
    A, B, Cc = cs.plant if mode in ("abc", "both") else cs.ins[:3]
    dist = cs.dist if mode in ("d", "both") else None
    nlt = cs.nl if "nlt" in given else None
    x, T = cs.ins[7].copy(), cs.ins[8].copy()
    ctl = aos(cs.c0).reshape(n, H, I) if "c" in given else None
    v = aos(cs.v0).reshape(n, H, I) if "v" in given else None
    keys = ("controls", "states", "sequences", "iters", "status", "rin", "rout")
    out = {k: [] for k in keys}
    with MpcSolver(horizon=H, device=None) as hs:
        for k in range(S):
            _, ctl, it, v = o.solve_general(I, H, *model, aos(x), aos(T).reshape(n, H, 2), controls_in=ctl, v_in=v,
                                            want_v=True)
            c = np.ascontiguousarray(ctl.reshape(n, H * I).T)
            st = ri = ro = None
            if polished:
                _, st, ri, ro = hs.polish_batch_general(*cs.ins[:7], x, T, c, tol=TOL, max_rounds=ROUNDS, inputs=I)
                ctl = aos(c).reshape(n, H, I)
            bu0, bu1 = B[0] * c[0], B[I] * c[0]
            if I == 2:
                bu0, bu1 = bu0 + B[1] * c[1], bu1 + B[3] * c[1]
            n0 = ((A[0] * x[0] + A[1] * x[1]) + bu0) + Cc[0]
            n1 = ((A[2] * x[0] + A[3] * x[1]) + bu1) + Cc[1]
            if dist is not None:
                n0, n1 = n0 + dist[2 * k], n1 + dist[2 * k + 1]
            x = np.stack([n0, n1])
            T[:-2] = T[2:].copy()
            if nlt is not None and k + 1 < S:
                T[-2:] = nlt[2 * (k + 1):2 * (k + 1) + 2]
            for name, val in zip(keys, (c[:I], x, c, it, st, ri, ro)):
                if val is not None:
                    out[name].append(np.array(val).reshape(-1, n))
    ref = {k: np.ascontiguousarray(np.concatenate(l)) for k, l in out.items() if l}
    ref["iters"] = ref["iters"].astype(np.int32)
    ref["c"], ref["v"] = c.copy(), np.ascontiguousarray(v.reshape(n, H * I).T)
    return ref


_REFS = {}


def ref_loop(cs, kind, mode, fallback, given):
    """{name: [rows, n]} of every output of the entry, and "flags" where the reference has them"""
    given = frozenset(given)
    key = (cs.key, kind, mode, fallback, given)
    if key in _REFS:
        return _REFS[key]
    if kind != "newton":
        ref = solve_loop(cs, kind == "polished", mode, given)
    elif fallback == "none":
        lib = capi.load_library()
        with MpcSolver(horizon=cs.H, device=None) as hs:
            rc, flags, out, _ = run_loop(lib, hs, cs, Mem(cs.n), "newton", mode, "none",
                                         (set(LOOP_OPTIONAL["newton"]) - {"c", "v", "nlt"}) | given)
        assert rc == capi.OK
        ref = {k: b.get() for k, b in out.items()}
        ref["flags"] = flags
    else:
        none, pol = ref_loop(cs, "newton", mode, "none", given), ref_loop(cs, "polished", mode, None, given)
        fbk = none["first"][0] < cs.S
        ref = {k: np.ascontiguousarray(np.where(fbk[None, :], pol[k], none[k])) for k in pol if k in none}
        ref["first"] = none["first"]
    _REFS[key] = ref
    return ref


def check_loop(cs, kind, mode, fallback, present, rc, flags, out, decoy):
    ref = ref_loop(cs, kind, mode, fallback, given_inputs(present))
    assert rc == capi.OK, rc
    _check_all(out, ref, decoy)
    if flags is None:
        return
    if "flags" in ref:
        assert flags == ref["flags"], (flags, ref["flags"])
    else:   # the solve-based loops: nothing is non-finite or a bad model here; NOT_POLISHED is the status rows'
        assert flags & (capi.FLAG_NONFINITE | capi.FLAG_BAD_MODEL) == 0, flags
        st = ref.get("status")
        if fallback == "solve":
            fbk = ref["first"][0] < cs.S
            assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((st[:, fbk] < 0).any()), flags
        elif st is not None:
            assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((st < 0).any()), flags


# ---- the derivative entries ------------------------------------------------------------------------------------------

GRAD_OUTS = ("dA", "dB", "dC", "dQ", "dR", "dlower", "dupper", "dx0", "dtargets", "dnew_last_targets", "kkt_residual")
PLANT_GRAD_OUTS = ("dAp", "dBp", "dCp", "ddisturbance")


def grad_rows(cs):
    I, H, S = cs.I, cs.H, cs.S
    return dict(dA=4, dB=2 * I, dC=2, dQ=2, dR=I, dlower=I, dupper=I, dx0=2, dtargets=2 * H, dnew_last_targets=2 * S,
                kkt_residual=1, dAp=4, dBp=2 * I, dCp=2, ddisturbance=2 * S)


def grad_outputs(mode, nlt=True):
    """every output the backward of this mode may be asked for"""
    outs = [k for k in GRAD_OUTS if nlt or k != "dnew_last_targets"]
    if mode in ("abc", "both"):
        outs += ["dAp", "dBp", "dCp"]
    return tuple(outs + (["ddisturbance"] if mode is not None else []))


def recorded(cs, mode):
    """(sequences, states) of the Newton loop in this mode: what the derivative entries are taken at"""
    r = ref_loop(cs, "newton", mode, "none", frozenset({"nlt"}))
    return r["sequences"], r["states"]


def run_backward(lib, s, cs, mem, mode, present, gu=True, gx=True, nlt=True, ld_d_zero=False, launch_only=False):
    """tpc_mpc_rollout_backward (mode None) or tpc_mpc_rollout_plant_backward with the outputs `present`:
    (rc, flags, {name: Buf}, decoy).  ld_d_zero: the plant's ld_d = 0, so ddisturbance has the io's ld."""
    rows = grad_rows(cs)
    io = _io(cs, mem)
    sq, xs = recorded(cs, mode)
    b = dict(sequences=mem.put(sq), states=mem.put(xs), grad_controls=mem.put(cs.G_u) if gu else None,
             grad_states=mem.put(cs.G_x) if gx else None)
    nl = mem.put(cs.nl) if nlt else None
    ld_dd = mem.ld if ld_d_zero else mem.ld_d
    out = {k: mem.out(rows[k], ld=ld_dd if k == "ddisturbance" else None) for k in present}
    decoy = mem.out(max(rows.values()))
    g = capi.RolloutGrad(**{k: _p(v) for k, v in b.items()}, **{k: _p(out.get(k)) for k in GRAD_OUTS})
    flags, p, st = C.c_uint32(99), s._params(), mem.stream_ptr()
    fl = None if launch_only else C.byref(flags)   # asking for the flags waits for the stream
    # the disturbance itself is not read
    pl = _plant(cs, mem, mode, with_dist=False, ld_d=0 if ld_d_zero else None) if mode is not None else None
    if mem.pending:
        mem.upload()
    if mode is None:
        rc = lib.tpc_mpc_rollout_backward(s._h, C.byref(p), C.byref(io), cs.S, _p(nl), C.byref(g), fl,
                                          mem.kind, st)
    else:
        pg = capi.PlantGrad(dA=_p(out.get("dAp")), dB=_p(out.get("dBp")), dC=_p(out.get("dCp")),
                            ddisturbance=_p(out.get("ddisturbance")))
        rc = lib.tpc_mpc_rollout_plant_backward(s._h, C.byref(p), C.byref(io), C.byref(pl), cs.S, _p(nl), C.byref(g),
                                                C.byref(pg), fl, mem.kind, st)
    if not launch_only:
        mem.sync()
    return rc, (None if launch_only else flags.value), out, decoy


def ref_backward(cs, mode, gu=True, gx=True, nlt=True):
    key = (cs.key, "backward", mode, gu, gx, nlt)
    if key not in _REFS:
        with MpcSolver(horizon=cs.H, device=None) as hs:
            rc, flags, out, _ = run_backward(capi.load_library(), hs, cs, Mem(cs.n), mode, grad_outputs(mode, nlt), gu,
                                             gx, nlt)
        assert rc == capi.OK and flags == 0, (rc, flags)
        _REFS[key] = {k: b.get() for k, b in out.items()}
    return _REFS[key]


def check_backward(cs, mode, rc, flags, out, decoy, **inputs):
    ref = ref_backward(cs, mode, **inputs)
    assert rc == capi.OK and flags in (0, None), (rc, flags)
    _check_all(out, ref, decoy)


TANGENTS = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "new_last_targets")
PLANT_TANGENTS = ("Ap", "Bp", "Cp", "disturbance")
TFIELDS = dict(A="tA", B="tB", C="tC", Q="tQ", R="tR", lower="tlower", upper="tupper", x0="tx0", targets="ttargets",
               new_last_targets="tnew_last_targets")


@functools.lru_cache(maxsize=None)
def _tangents(key, I, H, S, n, K):
    rng = np.random.default_rng(50 + K)
    rows = dict(A=4, B=2 * I, C=2, Q=2, R=I, lower=I, upper=I, x0=2, targets=2 * H, new_last_targets=2 * S, Ap=4,
                Bp=2 * I, Cp=2, disturbance=2 * S)
    return {k: rng.standard_normal((K * r, n)) for k, r in rows.items()}


def tangents(cs, K):
    """K directions of every tangent array, [K * rows, n] each"""
    return _tangents(cs.key, cs.I, cs.H, cs.S, cs.n, K)


def tangent_names(mode, single=False):
    names = [k for k in TANGENTS if not (single and k == "new_last_targets")]
    if mode in ("abc", "both"):
        names += ["Ap", "Bp", "Cp"]
    return tuple(names + (["disturbance"] if mode is not None else []))


def run_forward(lib, s, cs, mem, mode, K, given, want_states=True, single=False, ld_d_zero=False, launch_only=False):
    """tpc_mpc_rollout_forward (mode None), tpc_mpc_rollout_plant_forward, or (single) tpc_mpc_solve_batch_general_forward
    at the first recorded sequence, with the tangent arrays `given`: (rc, flags, {name: Buf}, decoy)"""
    I, H, S = cs.I, cs.H, cs.S
    io = _io(cs, mem)
    sq, xs = recorded(cs, mode)
    tan = tangents(cs, K)
    ld_td = mem.ld if ld_d_zero else mem.ld_d
    tb = {k: mem.put(tan[k], ld=ld_td if k == "disturbance" else None) for k in given}
    tt = capi.Tangents(directions=K, reserved=0, **{TFIELDS[k]: _p(tb.get(k)) for k in TANGENTS})
    flags, p, st = C.c_uint32(99), s._params(), mem.stream_ptr()
    fl = None if launch_only else C.byref(flags)   # asking for the flags waits for the stream
    decoy = mem.out(K * max(2 * S, H * I))
    if single:
        u = mem.put(np.ascontiguousarray(sq[:H * I]))
        out = dict(tcontrols=mem.out(K * H * I))
        if mem.pending:
            mem.upload()
        rc = lib.tpc_mpc_solve_batch_general_forward(s._h, C.byref(p), C.byref(io), u.ptr, C.byref(tt),
                                                     out["tcontrols"].ptr, fl, mem.kind, st)
    else:
        bs, bx, nl = mem.put(sq), mem.put(xs), mem.put(cs.nl)
        out = dict(tcontrols=mem.out(K * S * I))
        if want_states:
            out["tstates"] = mem.out(K * 2 * S)
        if mode is None:
            if mem.pending:
                mem.upload()
            rc = lib.tpc_mpc_rollout_forward(s._h, C.byref(p), C.byref(io), S, nl.ptr, bs.ptr, bx.ptr, C.byref(tt),
                                             out["tcontrols"].ptr, _p(out.get("tstates")), fl, mem.kind, st)
        else:
            pl = _plant(cs, mem, mode, with_dist=False, ld_d=0 if ld_d_zero else None)
            pt = capi.PlantTangents(tA=_p(tb.get("Ap")), tB=_p(tb.get("Bp")), tC=_p(tb.get("Cp")),
                                    tdisturbance=_p(tb.get("disturbance")))
            if mem.pending:
                mem.upload()
            rc = lib.tpc_mpc_rollout_plant_forward(s._h, C.byref(p), C.byref(io), C.byref(pl), S, nl.ptr, bs.ptr,
                                                   bx.ptr, C.byref(tt), C.byref(pt), out["tcontrols"].ptr,
                                                   _p(out.get("tstates")), fl, mem.kind, st)
    if not launch_only:
        mem.sync()
    return rc, (None if launch_only else flags.value), out, decoy


def ref_forward(cs, mode, K, given, single=False):
    key = (cs.key, "forward", mode, K, frozenset(given), single)
    if key not in _REFS:
        with MpcSolver(horizon=cs.H, device=None) as hs:
            rc, flags, out, _ = run_forward(capi.load_library(), hs, cs, Mem(cs.n), mode, K, given, True, single)
        assert rc == capi.OK and flags == 0, (rc, flags)
        _REFS[key] = {k: b.get() for k, b in out.items()}
    return _REFS[key]


def check_forward(cs, mode, K, given, single, rc, flags, out, decoy):
    ref = ref_forward(cs, mode, K, given, single)
    assert rc == capi.OK and flags in (0, None), (rc, flags)
    _check_all(out, ref, decoy)


# ---- the single polish (the side stream's second chain) --------------------------------------------------------------

def run_polish(lib, s, cs, mem, launch_only=False):
    """tpc_mpc_polish_batch_general from c0 with every output: (rc, flags, {name: Buf}, decoy)"""
    io = _io(cs, mem)
    out = dict(c=mem.put(cs.c0, fill=SENTINEL), u0=mem.out(cs.I), status=mem.out(1, integer=True), rin=mem.out(1),
               rout=mem.out(1))
    decoy = mem.out(cs.H * cs.I)
    io.controls_inout, io.u0 = out["c"].ptr, out["u0"].ptr
    q = capi.Polish(tol=TOL, max_rounds=ROUNDS, reserved=0, status=out["status"].ptr, residual_in=out["rin"].ptr,
                    residual_out=out["rout"].ptr)
    flags, p, st = C.c_uint32(99), s._params(), mem.stream_ptr()
    if mem.pending:
        mem.upload()
    rc = lib.tpc_mpc_polish_batch_general(s._h, C.byref(p), C.byref(io), C.byref(q),
                                          None if launch_only else C.byref(flags), mem.kind, st)
    if not launch_only:
        mem.sync()
    return rc, (None if launch_only else flags.value), out, decoy


def check_polish(cs, rc, flags, out, decoy):
    key = (cs.key, "polish")
    if key not in _REFS:
        with MpcSolver(horizon=cs.H, device=None) as hs:
            rc0, f0, o0, _ = run_polish(capi.load_library(), hs, cs, Mem(cs.n))
        assert rc0 == capi.OK
        _REFS[key] = dict({k: b.get() for k, b in o0.items()}, flags=f0)
    ref = _REFS[key]
    assert rc == capi.OK and flags in (ref["flags"], None), (rc, flags)
    _check_all(out, ref, decoy)
