"""CPU tests of the backward pass of the closed loop (tpc_mpc_rollout_backward): the dense closed-loop reference
(tests/model/mpc_rollout_dense.py) against finite differences of the oracle's closed loop, the host path of the entry
(a host-only handle runs the kernel's arithmetic on the calling thread) against the dense reference, the entry's
argument and flag behaviour, and the bits of the single-solve backward against the parent's (tests/golden)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle.bindings import Oracle
from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from trajectory_controller_amd import MpcSolver, capi

NAMES = rd.NAMES
KEY = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(eps=1e-12, max_iter=200000)


def _loss_grads(I, S, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, S, I)), rng.standard_normal((n, S, 2))


def _n_active_steps(I, H, th_i, seqs):
    return sum(int(dense.active(seqs[k], th_i["lo"], th_i["hi"]).any()) for k in range(len(seqs)))


@pytest.mark.parametrize("I,H,S,with_nlt", [(1, 4, 3, True), (2, 4, 12, False), (1, 1, 3, True), (2, 10, 12, True),
                                            (2, 10, 1, False), (1, 10, 12, False)])
def test_replay_and_dense_reference_against_finite_differences(I, H, S, with_nlt):
    """The replay reproduces Oracle.rollout bit for bit; the dense reference's autograd gradient matches central
    differences of the oracle's closed loop at eps 1e-12, on components whose perturbation changes no active set."""
    n = 4
    th, nlt = rd.batch(I, H, S, n, seed=2, with_nlt=with_nlt)
    G_u, G_x = _loss_grads(I, S, n, 11)
    checked = multi = 0
    for i in range(n):
        t0 = {k: np.array(th[k][i], dtype=np.float64) for k in NAMES}
        nl = None if nlt is None else nlt[i].copy()
        u0, xs, _, it = rd.replay(I, H, S, t0, nl)
        cu, cx, ci = Oracle().rollout(I, H, S, *[t0[k] for k in NAMES], new_last_targets=nl)
        assert np.array_equal(u0, cu) and np.array_equal(xs, cx) and np.array_equal(it, ci)
        _, _, seqs, _ = rd.replay(I, H, S, t0, nl, **TIGHT)
        acts = [dense.active(s, t0["lo"], t0["hi"]) for s in seqs]
        multi += int(_n_active_steps(I, H, t0, seqs) >= 2)
        ref, _, _, _ = rd.closed_loop(I, H, S, t0, nl, seqs, G_u[i], G_x[i])
        keys = list(NAMES) + (["nlt"] if nl is not None else [])
        for k in keys:
            arr = nl if k == "nlt" else t0[k]
            comps = np.arange(arr.size)
            if k == "Q":
                comps = comps[arr.ravel() != 0.0]
            if k in ("lo", "hi"):
                comps = comps[(t0["lo"] != t0["hi"])]
            if k == "nlt":
                comps = comps[2:]                       # row 0 is never read
            for c in comps[:6]:
                h = 1e-6 * max(1.0, abs(arr.ravel()[c]))
                vals, stable = [], True
                for sgn in (1.0, -1.0):
                    tp = {kk: vv.copy() for kk, vv in t0.items()}
                    nlp = None if nl is None else nl.copy()
                    (nlp if k == "nlt" else tp[k]).reshape(-1)[c] += sgn * h
                    a, b, sq, _ = rd.replay(I, H, S, tp, nlp, **TIGHT)
                    stable = stable and all(np.array_equal(dense.active(sq[kk], tp["lo"], tp["hi"]), acts[kk])
                                            for kk in range(S))
                    vals.append(rd.loss(a, b, G_u[i], G_x[i]))
                if not stable:
                    continue
                fd = (vals[0] - vals[1]) / (2 * h)
                want = ref[k].ravel()[c]
                assert abs(fd - want) <= 1e-4 * max(1.0, abs(want)), (i, k, c, fd, want)
                checked += 1
    assert checked >= 20, checked
    if S >= 3:
        assert multi >= 1


def _reference_batch(I, H, S, n, with_nlt, seed=0):
    """Inputs, the dense reference's closed loop (its sequences and states are the exact stationary points on the
    active sets of the oracle's closed loop at eps 1e-12) and its gradients; keep marks the instances whose stationary
    points keep the oracle's active sets."""
    th, nlt = rd.batch(I, H, S, n, seed=seed, with_nlt=with_nlt)
    G_u, G_x = _loss_grads(I, S, n, 5 + seed)
    refs, seqs, states, keep, nact = [], [], [], [], 0
    for i in range(n):
        t0 = {k: th[k][i] for k in NAMES}
        nl = None if nlt is None else nlt[i]
        _, _, sq, _ = rd.replay(I, H, S, t0, nl, **TIGHT)
        ref, _, xs, psq = rd.closed_loop(I, H, S, t0, nl, sq, G_u[i], G_x[i])
        keep.append(all(np.array_equal(dense.active(psq[k], t0["lo"], t0["hi"]), dense.active(sq[k], t0["lo"], t0["hi"]))
                        for k in range(S)))
        nact += int(_n_active_steps(I, H, t0, psq) >= 2)
        refs.append(ref)
        seqs.append(psq)
        states.append(xs)
    return th, nlt, G_u, G_x, refs, np.array(seqs), np.array(states), np.array(keep), nact


def _soa_inputs(I, H, S, th, nlt, G_u, G_x, seqs, states, n):
    ins = [dense.soa(th[k], n) for k in NAMES]
    return ins, (None if nlt is None else dense.soa(nlt, n)), dict(
        sequences=dense.soa(seqs, n), states=dense.soa(states, n), grad_controls=dense.soa(G_u, n),
        grad_states=dense.soa(G_x, n))


@pytest.mark.parametrize("I,H,S,with_nlt", [(1, 4, 9, True), (2, 4, 30, True), (2, 20, 6, True), (1, 20, 25, False),
                                            (2, 10, 10, False), (2, 1, 7, True), (1, 12, 30, True)])
def test_host_rollout_backward_matches_dense_reference(I, H, S, with_nlt):
    n = 6
    th, nlt, G_u, G_x, refs, seqs, states, keep, nact = _reference_batch(I, H, S, n, with_nlt)
    assert keep.sum() >= n // 2, keep
    ins, nl, g = _soa_inputs(I, H, S, th, nlt, G_u, G_x, seqs, states, n)
    with MpcSolver(horizon=H, device=None) as s:
        out = s.rollout_backward(S, *ins, nl, inputs=I, **g)
        assert s.last_flags == 0
    if with_nlt:
        assert np.all(out["new_last_targets"][:2] == 0.0)
    for i in np.flatnonzero(keep):
        for k in list(NAMES) + (["nlt"] if with_nlt else []):
            got = out["new_last_targets" if k == "nlt" else KEY[k]][:, i]
            want = refs[i][k].ravel()
            err = np.linalg.norm(got - want)
            assert err <= 1e-9 * np.linalg.norm(want) + 1e-12, f"instance {i} d{k}: |err| {err:.3e} " \
                f"|ref| {np.linalg.norm(want):.3e}"
        assert out["kkt_residual"][i] < 1e-8
    assert S < 3 or nact >= 1


# ---- ABI ----------------------------------------------------------------------------------------------------------

OUTS = ("dA", "dB", "dC", "dQ", "dR", "dlower", "dupper", "dx0", "dtargets", "dnew_last_targets", "kkt_residual")


def _rows(I, H, S):
    return dict(dA=4, dB=2 * I, dC=2, dQ=2, dR=I, dlower=I, dupper=I, dx0=2, dtargets=2 * H, dnew_last_targets=2 * S,
                kkt_residual=1)


def _wide_case(I, H, S, n, ld, pad=0.0):
    """SoA arrays with leading dimension ld (columns n.. are padding): inputs, nlt, sequences, states, G_u, G_x"""
    th, nlt = rd.batch(I, H, S, n, seed=3)
    seqs, states = [], []
    for i in range(n):
        _, xs, sq, _ = rd.replay(I, H, S, {k: th[k][i] for k in NAMES}, nlt[i], eps=1e-8, max_iter=20000)
        seqs.append(sq)
        states.append(xs)
    G_u, G_x = _loss_grads(I, S, n, 9)

    def wide(a):
        a = dense.soa(a, n)
        w = np.full((a.shape[0], ld), pad)
        w[:, :n] = a
        return w
    return ({k: wide(th[k]) for k in NAMES}, wide(nlt), wide(np.array(seqs)), wide(np.array(states)), wide(G_u),
            wide(G_x))


def _call(h, H, I, S, n, ld, case, outs, dtype=capi.F64, mem=capi.HOST, nlt=True, gu=True, gx=True, seq=True):
    ins, nl, sq, st, G_u, G_x = case
    p = capi.default_params(20, dtype=dtype)
    p.horizon = H
    ptr = lambda a: None if a is None else a.ctypes.data
    io = capi.GeneralIO(inputs=I, n=n, ld=ld, A=ptr(ins["A"]), B=ptr(ins["B"]), C=ptr(ins["C"]), Q=ptr(ins["Q"]),
                        R=ptr(ins["R"]), lower=ptr(ins["lo"]), upper=ptr(ins["hi"]), x0=ptr(ins["x0"]),
                        targets=ptr(ins["targets"]))
    gr = capi.RolloutGrad(sequences=ptr(sq) if seq else None, states=ptr(st), grad_controls=ptr(G_u) if gu else None,
                          grad_states=ptr(G_x) if gx else None, **{f: ptr(outs.get(f)) for f in OUTS})
    flags = C.c_uint32(0)
    lib = capi.load_library()
    rc = lib.tpc_mpc_rollout_backward(h, C.byref(p), C.byref(io), S, ptr(nl) if nlt else None, C.byref(gr),
                                      C.byref(flags), mem, None)
    return rc, flags.value


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


@pytest.mark.parametrize("I", [1, 2])
def test_rollout_backward_null_outputs_and_padding(host_handle, I):
    H, S, n, ld, sentinel = 5, 7, 9, 13, 12345.0
    case = _wide_case(I, H, S, n, ld, pad=np.nan)   # padding of the inputs is never read
    full = {f: np.full((r, ld), sentinel) for f, r in _rows(I, H, S).items()}
    rc, flags = _call(host_handle, H, I, S, n, ld, case, full)
    assert rc == 0 and flags == 0
    for f, a in full.items():
        assert np.all(a[:, n:] == sentinel), f"{f}: padding written"
        assert np.all(np.isfinite(a[:, :n])), f
    assert np.all(full["dnew_last_targets"][:2, :n] == 0.0)
    some = {f: np.full((r, ld), sentinel) for f, r in _rows(I, H, S).items() if f in ("dB", "dlower", "dtargets",
                                                                                       "dnew_last_targets")}
    rc, flags = _call(host_handle, H, I, S, n, ld, case, some)
    assert rc == 0 and flags == 0
    for f, a in some.items():
        assert np.array_equal(a, full[f]), f
    assert _call(host_handle, H, I, S, n, ld, case, {}) == (0, 0)
    # NULL grad_controls / grad_states are zeros
    zs = {f: np.zeros((r, ld)) for f, r in _rows(I, H, S).items()}
    zcase = case[:4] + (np.zeros_like(case[4]), np.zeros_like(case[5]))
    both = {f: np.full((r, ld), sentinel) for f, r in _rows(I, H, S).items()}
    assert _call(host_handle, H, I, S, n, ld, zcase, zs) == (0, 0)
    assert _call(host_handle, H, I, S, n, ld, case, both, gu=False, gx=False) == (0, 0)
    for f in zs:
        assert np.array_equal(both[f][:, :n], zs[f][:, :n]), f


@pytest.mark.parametrize("what,flag", [("targets", capi.FLAG_NONFINITE), ("nlt", capi.FLAG_NONFINITE),
                                       ("grad_states", capi.FLAG_NONFINITE), ("grad_controls", capi.FLAG_NONFINITE),
                                       ("sequences", capi.FLAG_NONFINITE), ("states", capi.FLAG_NONFINITE),
                                       ("R", capi.FLAG_BAD_MODEL), ("bounds", capi.FLAG_BAD_MODEL)])
def test_rollout_backward_flags_zero_the_instance(host_handle, what, flag):
    I, H, S, n = 2, 6, 8, 5
    case = _wide_case(I, H, S, n, n)
    clean = {f: np.empty((r, n)) for f, r in _rows(I, H, S).items()}
    assert _call(host_handle, H, I, S, n, n, case, clean) == (0, 0)
    ins, nl, sq, st, G_u, G_x = [dict((k, v.copy()) for k, v in case[0].items())] + [a.copy() for a in case[1:]]
    bad = 2
    if what == "targets":
        ins["targets"][3, bad] = np.nan
    elif what == "nlt":
        nl[2 * S - 1, bad] = np.inf
    elif what == "grad_states":
        G_x[5, bad] = np.nan
    elif what == "grad_controls":
        G_u[0, bad] = np.inf
    elif what == "sequences":
        sq[3 * H * I + 1, bad] = np.nan
    elif what == "states":
        st[2 * S - 1, bad] = np.nan
    elif what == "R":
        ins["R"][1, bad] = 0.0
    else:
        ins["hi"][0, bad] = ins["lo"][0, bad] - 0.1
    outs = {f: np.full((r, n), 7.0) for f, r in _rows(I, H, S).items()}
    rc, flags = _call(host_handle, H, I, S, n, n, (ins, nl, sq, st, G_u, G_x), outs)
    assert rc == 0 and flags == flag
    others = [k for k in range(n) if k != bad]
    for f, a in outs.items():
        assert np.all(a[:, bad] == 0.0), f
        assert np.array_equal(a[:, others], clean[f][:, others]), f


def test_rollout_backward_argument_errors(host_handle):
    I, H, S, n = 2, 4, 3, 3
    case = _wide_case(I, H, S, n, n)
    lib = capi.load_library()
    dn = {"dnew_last_targets": np.empty((2 * S, n))}
    rc, _ = _call(host_handle, H, I, S, n, n, case, dn, nlt=False)
    assert rc == 1 and b"new_last_targets" in lib.tpc_mpc_last_error(host_handle)
    rc, _ = _call(host_handle, H, I, S, n, n, case, {}, dtype=capi.F32)
    assert rc == 1 and b"fp64" in lib.tpc_mpc_last_error(host_handle)
    assert _call(host_handle, 65, I, S, n, n, case, {})[0] == 4
    assert _call(host_handle, H, I, S, n, n, case, {}, seq=False)[0] == 1
    assert _call(host_handle, H, I, S, n, n, case, {}, mem=capi.DEVICE)[0] == 6
    assert _call(host_handle, H, I, 0, n, n, case, {}) == (0, 0)
    assert _call(host_handle, H, I, S, 0, n, case, {}) == (0, 0)
    assert _call(host_handle, H, I, -1, n, n, case, {})[0] == 1


def test_single_solve_backward_bits_unchanged(host_handle):
    """The host path of tpc_mpc_solve_batch_general_backward on a fixed batch gives the bits recorded from the
    library before its arithmetic moved into the shared per-step core (tests/golden/grad_backward_bits.npz)."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "grad_backward_bits.npz"))
    lib = capi.load_library()
    for I, H in ((1, 9), (2, 12)):
        ins = {k: np.ascontiguousarray(gold[f"I{I}_in_{k}"]) for k in NAMES}
        u, g = np.ascontiguousarray(gold[f"I{I}_in_u"]), np.ascontiguousarray(gold[f"I{I}_in_g"])
        n = u.shape[1]
        names = ("dA", "dB", "dC", "dQ", "dR", "dlower", "dupper", "dx0", "dtargets", "kkt_residual")
        outs = {f: np.full(gold[f"I{I}_out_{f}"].shape, np.nan) for f in names}
        p = capi.default_params(20)
        p.horizon = H
        ptr = lambda a: a.ctypes.data
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(ins["A"]), B=ptr(ins["B"]), C=ptr(ins["C"]), Q=ptr(ins["Q"]),
                            R=ptr(ins["R"]), lower=ptr(ins["lo"]), upper=ptr(ins["hi"]), x0=ptr(ins["x0"]),
                            targets=ptr(ins["targets"]))
        gr = capi.GeneralGrad(controls=ptr(u), grad_controls=ptr(g), **{f: ptr(outs[f]) for f in names})
        flags = C.c_uint32(0)
        rc = lib.tpc_mpc_solve_batch_general_backward(host_handle, C.byref(p), C.byref(io), C.byref(gr),
                                                      C.byref(flags), capi.HOST, None)
        assert rc == 0 and flags.value == 0
        for f in names:
            assert outs[f].tobytes() == gold[f"I{I}_out_{f}"].tobytes(), (I, f)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_rollout_grad_kernel_has_no_scratch():
    """Both instantiations of the closed-loop backward kernel are in the library and touch no scratch memory at all
    (the per-step quantities live in the handle's workspace, lambda and the sums in registers)."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    assert check_loop_scratch.offenders(lib, ["rollout_grad_kernel"]) == []
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            for name, body in check_loop_scratch.kernels(co):
                if "rollout_grad_kernel" in name:
                    seen[name] = [t for _, t, _ in body if t.startswith("scratch_")]
    assert len(seen) == 2, sorted(seen)
    assert all(not hits for hits in seen.values()), {k: len(v) for k, v in seen.items()}
