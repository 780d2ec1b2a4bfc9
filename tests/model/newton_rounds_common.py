"""tests/model/newton_rounds_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What scripts/record_newton_rounds.py and the two tests of tests/golden/newton_rounds_parent.npz share: the shapes, how a
recorded case is run (on a host-only handle, or on a device handle in DEVICE memory), how two arrays are compared, and
what the recording must contain.  The recording holds, under "<case>/in/<name>", the inputs of a case and, under
"<case>/r<max_rounds>/<name>", what the library returned for them before the polish and the exact compact solve shared
one copy of the Newton rounds.

Cases: polish_I<I>_H<H> (tpc_mpc_polish_batch_general, arrays of LD columns of which N are the batch) and
<entry>_H<H> with entry one of COMPACT (tpc_mpc_solve_batch_compact_exact, _rows, _from without and with rows).
"""
import ctypes as C
import types

import numpy as np

from tests.model.compact_exact_common import NAMES
from trajectory_controller_amd import capi

HS = (1, 4, 5, 6)       # the degenerate loop, the two register kernels, the first horizon of the workspace kernel
N, LD = 67, 128         # one wavefront and three lanes; the polish's arrays are wider than the batch
TOL = 1e-9
POLISH_ROUNDS, COMPACT_ROUNDS = (8, 1), (16, 1)         # each entry's default, and one round
INPUTS = (1, 2)
COMPACT = ("cold", "cold_pinned", "rows", "warm", "warm_rows")
POLISH_OUT = ("controls", "u0", "status", "residual_in", "residual_out", "flags")
COMPACT_OUT = ("front", "rear", "sequence", "status", "residual_in", "residual_out", "flags")
SENTINEL = 12345.0


def inputs_of(gold, case):
    prefix = f"{case}/in/"
    return {k[len(prefix):]: gold[k] for k in gold.files if k.startswith(prefix)}


def same_bits(a, b):
    """equal bit for bit (fp64 as int64: signed zeros told apart, NaNs in the same places with the same payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        a, b = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
    return bool(np.array_equal(a, b))


class _Cuda:
    """a CUDA copy of a numpy array with the .ctypes.data a raw call reads its address from"""

    def __init__(self, a):
        import torch
        self.t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.ctypes = types.SimpleNamespace(data=self.t.data_ptr())

    def numpy(self):
        return self.t.cpu().numpy()


def run_polish(s, I, H, ins, rounds, device=False):
    """tpc_mpc_polish_batch_general of MpcSolver s on a recorded case, N columns of arrays LD wide: {name: whole array}
    of POLISH_OUT (the outputs start as sentinels, so the padding is compared too)"""
    wrap = _Cuda if device else (lambda a: np.array(a, order="C", copy=True))
    ptr = lambda a: a.ctypes.data
    bufs = {k: wrap(ins[k]) for k in NAMES}
    out = dict(controls=wrap(ins["controls"]), u0=wrap(np.full((I, LD), SENTINEL)),
               status=wrap(np.full(LD, -7, dtype=np.int32)), residual_in=wrap(np.full(LD, SENTINEL)),
               residual_out=wrap(np.full(LD, SENTINEL)))
    p = capi.default_params(H)
    io = capi.GeneralIO(inputs=I, n=N, ld=LD, A=ptr(bufs["A"]), B=ptr(bufs["B"]), C=ptr(bufs["C"]), Q=ptr(bufs["Q"]),
                        R=ptr(bufs["R"]), lower=ptr(bufs["lo"]), upper=ptr(bufs["hi"]), x0=ptr(bufs["x0"]),
                        targets=ptr(bufs["targets"]), controls_inout=ptr(out["controls"]), u0=ptr(out["u0"]))
    q = capi.Polish(tol=TOL, max_rounds=rounds, status=ptr(out["status"]), residual_in=ptr(out["residual_in"]),
                    residual_out=ptr(out["residual_out"]))
    flags = C.c_uint32(0)
    rc = capi.load_library().tpc_mpc_polish_batch_general(s._h, C.byref(p), C.byref(io), C.byref(q), C.byref(flags),
                                                          capi.DEVICE if device else capi.HOST, None)
    assert rc == 0, rc
    if device:
        import torch
        torch.cuda.synchronize()
        out = {k: b.numpy() for k, b in out.items()}
    out["flags"] = np.uint32(flags.value)
    return out


def run_compact(s, ins, rounds, device=False):
    """MpcSolver.solve_batch_compact_exact(fallback="none") on a recorded case: {name: array} of COMPACT_OUT.  The
    case's "lower" / "upper" override the solver's bounds, "params_rows" and "start" select the entry."""
    if device:
        import torch
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    else:
        up = lambda a: None if a is None else np.array(a, order="C", copy=True)
    over = {k: tuple(ins[k]) for k in ("lower", "upper") if k in ins}
    got = s.solve_batch_compact_exact(up(ins["v"]), up(ins["dy"]), up(ins["dphi"]), tol=TOL, max_rounds=rounds,
                                      fallback="none", want_sequence=True, want_residuals=True,
                                      params_rows=up(ins.get("params_rows")), start=up(ins.get("start")), **over)
    front, rear, seq, status, _, rin, rout = got
    if device:
        torch.cuda.synchronize()
    out = dict(front=front, rear=rear, sequence=seq, status=status, residual_in=rin, residual_out=rout)
    out = {k: np.ascontiguousarray(a.cpu().numpy() if device else a) for k, a in out.items()}
    out["flags"] = np.uint32(s.last_flags)
    return out


def families():
    """{family: [(case, its round limits)]}: the horizons of one entry together (cold_pinned is the cold entry)"""
    fam = {f"polish_I{I}": [(f"polish_I{I}_H{H}", POLISH_ROUNDS) for H in HS] for I in INPUTS}
    for e in COMPACT:
        fam.setdefault(e.split("_pinned")[0], []).extend((f"{e}_H{H}", COMPACT_ROUNDS) for H in HS)
    return fam


def check_contents(gold):
    """what the recorded rows must contain, per entry over its horizons: instances verified in round 0, in round 1
    and after three rounds or more, instances one round leaves unverified (status -1, flag 0x8), a non-finite instance
    (0x1), a bad-model instance (0x4, where the entry can have one: a shared model is rejected before the launch), a
    lower == upper component"""
    for family, cases in families().items():
        full = np.concatenate([gold[f"{c}/r{r[0]}/status"][:N] for c, r in cases])
        one = np.concatenate([gold[f"{c}/r{r[1]}/status"][:N] for c, r in cases])
        flags_full = np.bitwise_or.reduce([gold[f"{c}/r{r[0]}/flags"] for c, r in cases])
        flags_one = np.bitwise_or.reduce([gold[f"{c}/r{r[1]}/flags"] for c, r in cases])
        assert (full == 0).any() and (full == 1).any() and (full >= 3).any(), (family, np.bincount(full + 1))
        assert (one == -1).any() and flags_one & capi.FLAG_NOT_POLISHED, (family, np.bincount(one + 1), flags_one)
        assert flags_full & capi.FLAG_NONFINITE, (family, flags_full)
        per_instance_model = family.startswith("polish") or family.endswith("rows")
        assert bool(flags_full & capi.FLAG_BAD_MODEL) == per_instance_model, (family, flags_full)
        pinned = False
        for c, _ in cases:
            ins = inputs_of(gold, c)
            if "lo" in ins:
                pinned |= bool((ins["lo"][:, :N] == ins["hi"][:, :N]).any())
            elif "params_rows" in ins:
                pinned |= bool((ins["params_rows"][6:8] == ins["params_rows"][8:10]).any())
            else:
                pinned |= bool((ins["lower"] == ins["upper"]).any())
        assert pinned or family == "warm", family       # the shared model's pinned input is recorded cold
