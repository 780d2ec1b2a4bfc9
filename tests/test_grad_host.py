"""CPU tests of the backward pass of the general form (tpc_mpc_solve_batch_general_backward): the dense reference
(tests/model/mpc_grad_dense.py) against finite differences of the solved optimum, the host path of the entry (a
host-only handle runs the same arithmetic as the kernel on the calling thread) against the dense reference, and the
entry's argument and flag behaviour."""
import ctypes as C

import numpy as np
import pytest

from oracle.bindings import Oracle
from tests.model import mpc_grad_dense as dense
from trajectory_controller_amd import MpcSolver, capi

NAMES = dense.NAMES
KEY = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets")


def _grad_in(H, I, n, seed):
    return np.random.default_rng(seed).standard_normal((n, H, I))


def _host_backward(I, H, th, controls, g, **kw):
    n = controls.shape[0]
    with MpcSolver(horizon=H, device=None) as s:
        out = s.solve_batch_general_backward(*[dense.soa(th[k], n) for k in NAMES], dense.soa(controls, n),
                                             dense.soa(g, n), inputs=I, **kw)
        return out, s.last_flags


@pytest.mark.parametrize("I,H", [(1, 4), (2, 5), (2, 10)])
def test_dense_reference_matches_finite_differences(I, H):
    """The definition: central differences of the optimum on a stable active set (the oracle's solution at eps 1e-12,
    moved onto the exact stationary point of its active set) against the reference's autograd gradient.  Entries on
    the edge of the model's domain are left out: a zero Q (a step to either side leaves min(Q) >= 0) and the bounds of
    a pinned input (lower == upper: u is not differentiable there)."""
    n = 6
    th = dense.mixed_batch(I, H, n, seed=1)
    ctl, ustar, keep = dense.solved(I, H, th)
    g = _grad_in(H, I, n, 7)
    checked = 0
    for i in np.flatnonzero(keep):
        t0 = {k: th[k][i].astype(np.float64) for k in NAMES}
        act0 = dense.active(ctl[i], t0["lo"], t0["hi"])
        ref, _, _, _ = dense.instance(I, H, t0, ustar[i], g[i])
        edge = {k: np.zeros(t0[k].size, dtype=bool) for k in NAMES}
        edge["Q"] = t0["Q"] == 0.0
        edge["lo"] = edge["hi"] = t0["lo"] == t0["hi"]
        ref_all = np.concatenate([ref[k].ravel()[~edge[k]] for k in NAMES])
        fd_all = []
        stable = True
        for k in NAMES:
            flat = t0[k].ravel()
            for c in np.flatnonzero(~edge[k]):
                h = 1e-6 * max(1.0, abs(flat[c]))
                vals = []
                for sgn in (1.0, -1.0):
                    tp = {kk: vv.copy() for kk, vv in t0.items()}
                    tp[k].reshape(-1)[c] += sgn * h
                    _, cp, _ = Oracle().solve_general(I, H, *[tp[kk][None] for kk in NAMES], eps=1e-12, max_iter=200000)
                    if not np.array_equal(dense.active(cp[0], tp["lo"], tp["hi"]), act0):
                        stable = False
                    vals.append(float(np.sum(dense.optimum_on(I, H, tp, cp[0]) * g[i])))
                fd_all.append((vals[0] - vals[1]) / (2 * h))
        if not stable:
            continue
        fd_all = np.array(fd_all)
        err = np.linalg.norm(fd_all - ref_all) / np.linalg.norm(ref_all)
        assert err < 1e-5, (i, err)
        checked += 1
    assert checked >= 3, checked


@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H", [1, 2, 4, 5, 10, 20, 33, 40, 64])
def test_host_backward_matches_dense_reference(I, H):
    n = 12
    th = dense.mixed_batch(I, H, n)
    _, ustar, keep = dense.solved(I, H, th)
    assert keep.sum() >= n // 2, keep
    g = _grad_in(H, I, n, 3)
    out, flags = _host_backward(I, H, th, ustar, g)
    assert flags == 0
    n_act = n_both = 0
    for i in np.flatnonzero(keep):
        t0 = {k: th[k][i] for k in NAMES}
        ref, _, cond, act = dense.instance(I, H, t0, ustar[i], g[i])
        n_act += int(act.any())
        n_both += int(act.all(axis=1).any()) if I == 2 else 0
        for k in NAMES:
            got = out[KEY[k]][:, i]
            want = ref[k].ravel()
            err = np.linalg.norm(got - want)
            assert err <= 1e-8 * np.linalg.norm(want) + 1e-300, f"instance {i} d{k}: |err| {err:.3e} |ref| " \
                f"{np.linalg.norm(want):.3e} cond(H_FF) {cond:.3e}"
        assert out["kkt_residual"][i] < 1e-9
    assert n_act > 0 and (I == 1 or n_both > 0)


def _io_arrays(I, H, n, ld, pad=0.0):
    """SoA arrays with leading dimension ld (columns n.. are padding)"""
    th = dense.mixed_batch(I, H, n)
    _, ustar, _ = dense.solved(I, H, th, eps=1e-10, max_iter=20000)
    g = _grad_in(H, I, n, 5)

    def wide(a):
        a = dense.soa(a, n)
        w = np.full((a.shape[0], ld), pad)
        w[:, :n] = a
        return w
    return {k: wide(th[k]) for k in NAMES}, wide(ustar), wide(g)


def _call(h, H, I, n, ld, ins, u, g, outs, dtype=capi.F64, mem=capi.HOST, controls=True):
    p = capi.default_params(H if 1 <= H <= 64 else 20, dtype=dtype)
    p.horizon = H
    ptr = lambda a: None if a is None else a.ctypes.data
    io = capi.GeneralIO(inputs=I, n=n, ld=ld, A=ptr(ins["A"]), B=ptr(ins["B"]), C=ptr(ins["C"]), Q=ptr(ins["Q"]),
                        R=ptr(ins["R"]), lower=ptr(ins["lo"]), upper=ptr(ins["hi"]), x0=ptr(ins["x0"]),
                        targets=ptr(ins["targets"]))
    gr = capi.GeneralGrad(controls=ptr(u) if controls else None, grad_controls=ptr(g),
                          **{f: ptr(outs.get(f)) for f in ("dA", "dB", "dC", "dQ", "dR", "dlower", "dupper", "dx0",
                                                          "dtargets", "kkt_residual")})
    flags = C.c_uint32(0)
    lib = capi.load_library()
    rc = lib.tpc_mpc_solve_batch_general_backward(h, C.byref(p), C.byref(io), C.byref(gr), C.byref(flags), mem, None)
    return rc, flags.value


def _rows(I, H):
    return dict(dA=4, dB=2 * I, dC=2, dQ=2, dR=I, dlower=I, dupper=I, dx0=2, dtargets=2 * H, kkt_residual=1)


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


@pytest.mark.parametrize("I", [1, 2])
def test_backward_null_outputs_and_padding(host_handle, I):
    H, n, ld, sentinel = 7, 9, 13, 12345.0
    ins, u, g = _io_arrays(I, H, n, ld, pad=np.nan)   # padding of the inputs is never read
    full = {f: np.full((r, ld), sentinel) for f, r in _rows(I, H).items()}
    rc, flags = _call(host_handle, H, I, n, ld, ins, u, g, full)
    assert rc == 0 and flags == 0
    for f, a in full.items():
        assert np.all(a[:, n:] == sentinel), f"{f}: padding written"
        assert np.all(np.isfinite(a[:, :n])), f
    # the same call with every other output NULL: the given ones are the same bits, nothing else is touched
    some = {f: np.full((r, ld), sentinel) for f, r in _rows(I, H).items() if f in ("dB", "dlower", "dtargets")}
    rc, flags = _call(host_handle, H, I, n, ld, ins, u, g, some)
    assert rc == 0 and flags == 0
    for f, a in some.items():
        assert np.array_equal(a, full[f]), f
    # and with no output at all
    assert _call(host_handle, H, I, n, ld, ins, u, g, {}) == (0, 0)


@pytest.mark.parametrize("what,flag", [("targets", capi.FLAG_NONFINITE), ("grad", capi.FLAG_NONFINITE),
                                       ("controls", capi.FLAG_NONFINITE), ("R", capi.FLAG_BAD_MODEL),
                                       ("bounds", capi.FLAG_BAD_MODEL)])
def test_backward_flags_zero_the_instance(host_handle, what, flag):
    I, H, n = 2, 6, 5
    ins, u, g = _io_arrays(I, H, n, n)
    clean = {f: np.empty((r, n)) for f, r in _rows(I, H).items()}
    assert _call(host_handle, H, I, n, n, ins, u, g, clean) == (0, 0)
    bad = 2
    if what == "targets":
        ins["targets"][3, bad] = np.nan
    elif what == "grad":
        g[H * I - 1, bad] = np.inf
    elif what == "controls":
        u[0, bad] = np.nan
    elif what == "R":
        ins["R"][1, bad] = 0.0
    else:
        ins["hi"][0, bad] = ins["lo"][0, bad] - 0.1
    outs = {f: np.full((r, n), 7.0) for f, r in _rows(I, H).items()}
    rc, flags = _call(host_handle, H, I, n, n, ins, u, g, outs)
    assert rc == 0 and flags == flag
    for f, a in outs.items():
        assert np.all(a[:, bad] == 0.0), f
        others = [k for k in range(n) if k != bad]
        assert np.array_equal(a[:, others], clean[f][:, others]), f


def test_backward_argument_errors(host_handle):
    I, H, n = 2, 4, 3
    ins, u, g = _io_arrays(I, H, n, n)
    lib = capi.load_library()
    rc, _ = _call(host_handle, H, I, n, n, ins, u, g, {}, dtype=capi.F32)
    assert rc == 1 and b"fp64" in lib.tpc_mpc_last_error(host_handle)
    assert _call(host_handle, 65, I, n, n, ins, u, g, {})[0] == 4
    assert _call(host_handle, H, I, n, n, ins, u, g, {}, controls=False)[0] == 1
    assert _call(host_handle, H, I, n, n, ins, u, g, {}, mem=capi.DEVICE)[0] == 6
