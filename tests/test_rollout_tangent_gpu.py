"""GPU tests of the forward-mode derivatives (tpc_mpc_rollout_forward, tpc_mpc_solve_batch_general_forward,
torch.autograd.forward_ad through mpc_rollout / mpc_general / mpc_compact): the gfx950 kernels equal the host-only
handle bit for bit, the transpose identity against the device backward, central differences of rollout_newton, the
jvp of the autograd functions, the existing entries are untouched, and one full-size run."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.autograd.forward_ad as fwAD

from tests.model import mpc_rollout_tangent_dense as td
from tests.test_rollout_newton_host import COVERAGE_CAP, inputs, soa_inputs
from tests.test_rollout_tangent_host import BOUND, CASES, identity_mismatch, mismatch, recorded_case
from trajectory_controller_amd import MpcSolver, capi, mpc_compact, mpc_general, mpc_rollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _single(tan):
    return {k: v for k, v in tan.items() if k != "new_last_targets"}


def _both(s, I, H, S, ins, nl, sq, st, tan, conv=lambda a: a):
    """(tcontrols, tstates) of the closed loop and tcontrols of the single solve at step 0's sequence, as numpy"""
    c = lambda a: None if a is None else conv(a)
    dins, ctan = [c(a) for a in ins], {k: c(v) for k, v in tan.items()}
    tu, tx = s.rollout_forward(S, *dins, c(nl), sequences=c(sq), states=c(st), tangents=ctan, inputs=I)
    f1 = s.last_flags
    tw = s.solve_batch_general_forward(*dins, c(np.ascontiguousarray(sq[:H * I])), _single(ctan), inputs=I)
    return [np.ascontiguousarray(_np(a)) for a in (tu, tx, tw)], f1 | s.last_flags


# every I x H of {1, 2} x {4, 10, 20, 40}, H = 1 and H = 64 once; n = 70 and 333 are no multiple of 64, so wavefronts
# straddle the boundary between two directions; K = 1 and 3; with and without new_last_targets
BITS = [(1, 4, 5, 70, 1, True), (2, 4, 4, 333, 3, False), (1, 10, 4, 333, 3, True), (2, 10, 5, 70, 1, False),
        (1, 20, 3, 70, 3, False), (2, 20, 4, 333, 1, True), (1, 40, 3, 333, 1, False), (2, 40, 3, 70, 3, True),
        (2, 1, 4, 70, 3, True), (2, 64, 2, 333, 1, False)]


@pytest.mark.parametrize("I,H,S,n,K,with_nlt", BITS)
def test_device_equals_host_only_handle_bits(I, H, S, n, K, with_nlt):
    ins, nl, sq, st, *_ = recorded_case(I, H, S, n, with_nlt, seed=4)
    tan = td.soa_tangents(td.random_tangents(I, H, S, n, 6, with_nlt=with_nlt, K=K), n)
    with MpcSolver(horizon=H, device=None) as s:
        want, wf = _both(s, I, H, S, ins, nl, sq, st, tan)
    with MpcSolver(horizon=H, device=0) as s:
        host, hf = _both(s, I, H, S, ins, nl, sq, st, tan)            # HOST memory, staged
        dev, df = _both(s, I, H, S, ins, nl, sq, st, tan, conv=up)    # DEVICE memory
    assert wf == hf == df == 0
    for name, w, a, b in zip(("tcontrols", "tstates", "single"), want, host, dev):
        assert w.shape == a.shape == b.shape and np.isfinite(w).all() and w.any(), name
        assert w.tobytes() == a.tobytes(), name + " (HOST)"
        assert w.tobytes() == b.tobytes(), name + " (DEVICE)"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_shard_of_a_wider_batch(device):
    """ld > n through the C entries: a shard's outputs equal the packed call's, the padding is untouched"""
    I, H, S, n, k0, m, K = 2, 10, 4, 200, 37, 70, 3
    ins, nl, sq, st, *_ = recorded_case(I, H, S, n, True, seed=5)
    tan = td.soa_tangents(td.random_tangents(I, H, S, n, 7, K=K), n)
    cut = lambda a: np.ascontiguousarray(a[..., k0:k0 + m])
    with MpcSolver(horizon=H, device=None) as s:
        want, _ = _both(s, I, H, S, [cut(a) for a in ins], cut(nl), cut(sq), cut(st), {k: cut(v) for k, v in tan.items()})
    lib = capi.load_library()
    sentinel = 777.0
    conv = up if device else (lambda a: a)
    off = (lambda t: t.data_ptr() + t.element_size() * k0) if device else (lambda a: a.ctypes.data + a.itemsize * k0)
    fields = dict(A="tA", B="tB", C="tC", Q="tQ", R="tR", lower="tlower", upper="tupper", x0="tx0",
                  targets="ttargets", new_last_targets="tnew_last_targets")
    with MpcSolver(horizon=H, device=0) as s:
        p = s._params()
        dins, dnl, dsq, dst = [conv(a) for a in ins], conv(nl), conv(sq), conv(st)
        dtan = {k: conv(v) for k, v in tan.items()}
        tu, tx, tw = (conv(np.full((K * r, n), sentinel)) for r in (S * I, 2 * S, H * I))
        io = capi.GeneralIO(inputs=I, n=m, ld=n, A=off(dins[0]), B=off(dins[1]), C=off(dins[2]), Q=off(dins[3]),
                            R=off(dins[4]), lower=off(dins[5]), upper=off(dins[6]), x0=off(dins[7]),
                            targets=off(dins[8]))
        tt = capi.Tangents(directions=K, reserved=0, **{fields[k]: off(v) for k, v in dtan.items()})
        flags = C.c_uint32(9)
        mem = capi.DEVICE if device else capi.HOST
        assert lib.tpc_mpc_rollout_forward(s._h, C.byref(p), C.byref(io), S, off(dnl), off(dsq), off(dst), C.byref(tt),
                                           off(tu), off(tx), C.byref(flags), mem, None) == 0 and flags.value == 0
        assert lib.tpc_mpc_solve_batch_general_forward(s._h, C.byref(p), C.byref(io), off(dsq), C.byref(tt), off(tw),
                                                       C.byref(flags), mem, None) == 0 and flags.value == 0
        if device:
            torch.cuda.synchronize()
    for got, w in zip((tu, tx, tw), want):
        got = _np(got)
        assert np.ascontiguousarray(got[:, k0:k0 + m]).tobytes() == w.tobytes()
        assert np.all(got[:, :k0] == sentinel) and np.all(got[:, k0 + m:] == sentinel)


# ---- derivatives -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_nlt", [True, False], ids=["nlt", "nonlt"])
@pytest.mark.parametrize("I,H,S", CASES)
def test_transpose_identity_against_the_device_backward(I, H, S, with_nlt):
    with MpcSolver(horizon=H, device=0) as s:
        worst = identity_mismatch(s, I, H, S, 40, with_nlt, to=up, back=_np)
    print(f"I={I} H={H} S={S} nlt={with_nlt}: largest mismatch {worst:.3e} (bound {BOUND:.3e})")
    assert worst <= BOUND, worst


@pytest.mark.parametrize("I,H,S", [(2, 10, 8), (1, 20, 6)])
def test_rollout_forward_matches_central_differences_of_rollout_newton(I, H, S):
    """One direction per entry of Q, R and x0 (K = 4 + I), all in one call, against central differences of the loop
    itself.  tol = 1e-12 and h = 1e-6 keep tol / h two orders under the asserted 1e-4
    (tests/test_rollout_polish_gpu.py::test_autograd_matches_finite_differences_of_the_polished_loop, whose assertion
    this is); instances the Newton pass does not carry at the base point or at a perturbed one are left out."""
    n, tol, h, rounds = 40, 1e-12, 1e-6, 8
    th, nlt = inputs("general", I, H, S)
    ins, nl = soa_inputs(th, nlt, n)
    dirs = [(3, "Q", r) for r in range(2)] + [(4, "R", r) for r in range(I)] + [(7, "x0", r) for r in range(2)]
    K = len(dirs)
    tan = {name: np.zeros((K, ins[idx].shape[0], n)) for idx, name, _ in dirs}
    for d, (idx, name, r) in enumerate(dirs):
        tan[name][d, r] = 1.0
    with MpcSolver(horizon=H, device=0) as s:
        def loop(vals):
            u, x, q, _, _, first = s.rollout_newton(S, *[up(a) for a in vals], up(nl), inputs=I, tol=tol,
                                                    max_rounds=rounds, fallback="none")
            return _np(u), _np(x), q, _np(first) == S
        u, x, q, carried = loop(ins)
        assert 1.0 - carried.mean() <= COVERAGE_CAP
        tu, tx = s.rollout_forward(S, *[up(a) for a in ins], up(nl), sequences=q, states=up(x),
                                   tangents={k: up(v) for k, v in tan.items()}, inputs=I)
        assert s.last_flags == 0
        tu, tx = _np(tu), _np(tx)
        checked = used = 0
        for d, (idx, name, r) in enumerate(dirs):
            vp, vm = [a.copy() for a in ins], [a.copy() for a in ins]
            vp[idx][r] += h
            vm[idx][r] -= h
            (pu, px, _, okp), (mu, mx, _, okm) = loop(vp), loop(vm)
            use = carried & okp & okm
            if name == "Q":   # a zero Q is the edge of the model's domain
                use = use & (ins[idx][r] != 0.0)
            ok = np.ones(n, dtype=bool)
            for fd, got in (((pu - mu) / (2 * h), tu[d]), ((px - mx) / (2 * h), tx[d])):
                ok &= (np.abs(fd - got) <= 1e-4 * np.maximum(1.0, np.abs(got))).all(axis=0)
            assert use.sum() == 0 or ok[use].mean() >= 0.8, (name, r)   # an active set may move
            checked += int(ok[use].sum())
            used += int(use.sum())
        print(f"I={I} H={H} S={S}: {used} (direction, instance) pairs compared, {checked} within 1e-4")
        assert used >= 0.5 * K * n and checked >= 0.8 * used, (used, checked)


def _dual_run(fn, leaves, tangents):
    """fn on dual tensors made of (leaves, tangents); (primal outputs, tangent outputs), each a tuple"""
    with fwAD.dual_level():
        duals = [fwAD.make_dual(a, t) if t is not None else a for a, t in zip(leaves, tangents)]
        outs = fn(*duals)
        outs = outs if isinstance(outs, tuple) else (outs,)
        un = [fwAD.unpack_dual(o) for o in outs]
        return tuple(u.primal.clone() for u in un), tuple(u.tangent.clone() for u in un)


@pytest.mark.parametrize("I,H,S,with_nlt", [(2, 10, 8, True), (1, 20, 5, False)])
def test_forward_ad_through_mpc_rollout(I, H, S, with_nlt):
    n = 40
    th, nlt = inputs("general", I, H, S, with_nlt=with_nlt)
    ins, nl = soa_inputs(th, nlt, n)
    rng = np.random.default_rng(8)
    names = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets") + (("new_last_targets",) if with_nlt else ())
    leaves = [up(a) for a in ins] + ([up(nl)] if with_nlt else [])
    tans = [up(rng.standard_normal(tuple(a.shape))) for a in leaves]
    tans[2] = None     # an input without a tangent arrives as None
    with MpcSolver(horizon=H, device=0) as s:
        fn = lambda *a: mpc_rollout(s, S, *a[:9], new_last_targets=a[9] if with_nlt else None, polish=True,
                                    newton_first=True)
        (u, x), (tu, tx) = _dual_run(fn, leaves, tans)
        cu, cx, cq, *_ = s.rollout_newton(S, *leaves[:9], leaves[9] if with_nlt else None, inputs=I, want_status=False)
        assert _np(u).tobytes() == _np(cu).tobytes() and _np(x).tobytes() == _np(cx).tobytes()
        du, dx = s.rollout_forward(S, *leaves[:9], leaves[9] if with_nlt else None, sequences=cq, states=cx, inputs=I,
                                   tangents={k: t for k, t in zip(names, tans) if t is not None})
        assert _np(tu).tobytes() == _np(du[0]).tobytes() and _np(tx).tobytes() == _np(dx[0]).tobytes()
        # ... and agrees with backward through the identity
        req = [a.clone().requires_grad_(True) for a in leaves]
        G_u, G_x = up(rng.standard_normal(tuple(u.shape))), up(rng.standard_normal(tuple(x.shape)))
        ru, rx = fn(*req)
        grads = torch.autograd.grad((ru * G_u).sum() + (rx * G_x).sum(), req)
    m = mismatch([_np(G_u * tu), _np(G_x * tx)], [_np(g * t) for g, t in zip(grads, tans) if t is not None])
    assert m.max() <= BOUND, m.max()


@pytest.mark.parametrize("I,H", [(2, 10), (1, 20)])
def test_forward_ad_through_mpc_general(I, H):
    n = 40
    th, _ = inputs("general", I, H, 1, with_nlt=False)
    ins, _ = soa_inputs(th, None, n)
    rng = np.random.default_rng(9)
    names = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets")
    leaves = [up(a) for a in ins]
    tans = [up(rng.standard_normal(a.shape)) for a in ins]
    tans[0] = None
    with MpcSolver(horizon=H, device=0) as s:
        fn = lambda *a: mpc_general(s, *a, polish=True)
        (u,), (tu,) = _dual_run(fn, leaves, tans)
        direct = s.solve_batch_general_forward(*leaves, u, {k: t for k, t in zip(names, tans) if t is not None},
                                               inputs=I)
        assert _np(tu).tobytes() == _np(direct[0]).tobytes() and _np(tu).any()
        req = [a.clone().requires_grad_(True) for a in leaves]
        G = up(rng.standard_normal(tuple(u.shape)))
        grads = torch.autograd.grad((fn(*req) * G).sum(), req)
    m = mismatch([_np(G * tu)], [_np(g * t) for g, t in zip(grads, tans) if t is not None])
    assert m.max() <= BOUND, m.max()


def test_forward_ad_through_mpc_compact():
    """a tangent of the four weights through the torch ops that build the model, then the jvp of mpc_general: equal to
    the direct call on that model, and the transpose of backward"""
    H, n = 10, 64
    rng = np.random.default_rng(10)
    v, dy, dphi = up(rng.uniform(0.5, 2.0, n)), up(0.2 * rng.standard_normal(n)), up(0.2 * rng.standard_normal(n))
    w = up(rng.uniform(0.5, 2.0, (4, n)))
    tw = up(rng.standard_normal((4, n)))
    with MpcSolver(horizon=H, device=0) as s:
        fn = lambda w_: mpc_compact(s, v, dy, dphi, w_, polish=True)
        (f, r), (tf, tr) = _dual_run(fn, [w], [tw])
        # the model mpc_compact builds (trajectory_controller_amd/autograd.py), and the direct call on it
        a = 22.0 * np.pi / 180.0
        T, l = torch.as_tensor(0.1, dtype=v.dtype, device=DEV), torch.as_tensor(0.21, dtype=v.dtype, device=DEV)
        Tv, one, zero = T * v, torch.ones_like(v), torch.zeros_like(v)     # tensor operands, as mpc_compact has them
        model = [torch.stack([one, Tv, zero, one]), torch.stack([zero, Tv, Tv / l, -Tv / l]), torch.zeros_like(w[:2]),
                 w[0:2].contiguous(), w[2:4].contiguous(), torch.full_like(w[:2], -a), torch.full_like(w[:2], a),
                 torch.zeros_like(w[:2]), torch.stack([dy, dphi]).repeat(H, 1)]
        u = mpc_general(s, *model, polish=True)
        assert _np(u[0]).tobytes() == _np(f).tobytes() and _np(u[1]).tobytes() == _np(r).tobytes()
        direct = s.solve_batch_general_forward(*model, u, {"Q": tw[0:2].contiguous(), "R": tw[2:4].contiguous()},
                                               inputs=2)
        assert _np(direct[0, 0]).tobytes() == _np(tf).tobytes() and _np(direct[0, 1]).tobytes() == _np(tr).tobytes()
        assert _np(tf).any()
        wr = w.clone().requires_grad_(True)
        Gf, Gr = up(rng.standard_normal(n)), up(rng.standard_normal(n))
        rf, rr = fn(wr)
        (gw,) = torch.autograd.grad((rf * Gf).sum() + (rr * Gr).sum(), [wr])
    m = mismatch([_np(Gf * tf)[None], _np(Gr * tr)[None]], [_np(gw * tw)])
    assert m.max() <= BOUND, m.max()


# ---- the existing entries --------------------------------------------------------------------------------------------

def test_existing_entries_untouched_by_a_tangent_call():
    """rollout_record, rollout_backward, polish_batch_general and rollout_newton before and after the forward-mode
    calls on the same handle: the same bytes (they share the staging buffer and the gradient workspace)"""
    I, H, S, n, K = 2, 10, 6, 300, 3
    ins, nl, sq, st, *_ = recorded_case(I, H, S, n, True, seed=7)
    tan = td.soa_tangents(td.random_tangents(I, H, S, n, 8, K=K), n)
    dins, dnl = [up(a) for a in ins], up(nl)
    with MpcSolver(horizon=H, device=0) as s:
        def existing():
            outs = list(s.rollout_record(S, *dins, dnl, inputs=I, want_iters=True))
            g = s.rollout_backward(S, *dins, dnl, sequences=outs[2], states=outs[1], grad_states=torch.ones_like(outs[1]),
                                   inputs=I)
            outs += [g[k] for k in sorted(g)]
            c = outs[2][:H * I].clone()
            outs += [c] + list(s.polish_batch_general(*dins, c, inputs=I))
            outs += list(s.rollout_newton(S, *dins, dnl, inputs=I, want_iters=True))
            outs += list(s.rollout_newton(S, *ins, nl, inputs=I, fallback="none"))
            torch.cuda.synchronize()
            return [np.ascontiguousarray(_np(a)).tobytes() for a in outs if a is not None]
        before = existing()
        _both(s, I, H, S, ins, nl, sq, st, tan, conv=up)
        mid = existing()
        _both(s, I, H, S, ins, nl, sq, st, tan)
        after = existing()
    assert before == mid == after


# ---- full size -------------------------------------------------------------------------------------------------------

FULL = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from trajectory_controller_amd import MpcSolver
from trajectory_controller_amd.synth import general_inputs
from tests.test_rollout_tangent_host import BOUND, mismatch
H, n, S, I, K, m = 20, 262144, 10, 2, 4, 1024
g = general_inputs(H, n, I=I, seed=5)
names = ["A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets"]
ins = [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).to("cuda:0") for k in names]
rng = np.random.default_rng(1)
tan = {"Q": torch.from_numpy(rng.standard_normal((K, 2, n))).to("cuda:0"),
       "R": torch.from_numpy(rng.standard_normal((K, I, n))).to("cuda:0")}
with MpcSolver(horizon=H, device=0) as s:
    u, x, q, *_ = s.rollout_newton(S, *ins, inputs=I, want_status=False)
    tu, tx = s.rollout_forward(S, *ins, sequences=q, states=x, tangents=tan, inputs=I)
    torch.cuda.synchronize()
    flags = s.last_flags
    finite = bool(torch.isfinite(tu).all() and torch.isfinite(tx).all())
    print("flags", flags, "finite", finite, "max |tu|", float(tu.abs().max()), "max |tx|", float(tx.abs().max()))
    assert flags == 0 and finite and tuple(tu.shape) == (K, S * I, n) and tuple(tx.shape) == (K, S * 2, n)
    # the identity on a sample: the backward on the sample's columns against the big run's tangents
    cols = torch.from_numpy(np.sort(rng.choice(n, m, replace=False))).to("cuda:0")
    cut = lambda a: a.index_select(-1, cols).contiguous()
    G_u, G_x = torch.from_numpy(rng.standard_normal((S * I, m))).to("cuda:0"), \
        torch.from_numpy(rng.standard_normal((2 * S, m))).to("cuda:0")
    gr = s.rollout_backward(S, *[cut(a) for a in ins], sequences=cut(q), states=cut(x), grad_controls=G_u,
                            grad_states=G_x, inputs=I, want=("Q", "R"))
    assert s.last_flags == 0
    worst = 0.0
    for d in range(K):
        mm = mismatch([(G_u * cut(tu[d])).cpu().numpy(), (G_x * cut(tx[d])).cpu().numpy()],
                      [(gr[k] * cut(tan[k][d])).cpu().numpy() for k in tan])
        worst = max(worst, float(mm.max()))
    print("identity on", m, "instances: largest mismatch", worst, "bound", BOUND)
    assert 0.0 < worst <= BOUND
"""


def test_full_size_run():
    """262 144 x N = 20 x 10 steps x K = 4, two inputs, DEVICE memory, once, in a child process under its own time
    limit: finite outputs, no flags, and the transpose identity on a 1 024-instance sample"""
    r = subprocess.run([sys.executable, "-c", FULL, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
