"""GPU tests of the polished closed loop (tpc_mpc_rollout_polished, MpcSolver.rollout_polished,
mpc_rollout(polish=True)): the fused polish + step kernel equals the composition of the public entries bit for bit,
a shard of a wider batch, max_rounds = 0, the existing closed loops are untouched, every step is the optimum (the
dense closed loop on the polished sequences' active sets), the gradients, the flags, and one full-size run."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.model import mpc_rollout_polish_ref as rp
from tests.test_rollout_polish_host import BOUND, CAP, CASES, ROUNDS, TOL
from trajectory_controller_amd import MpcSolver, capi, mpc_rollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = rd.NAMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets")


def _case(I, H, S, n, seed, with_nlt=True):
    """component-major numpy inputs of mpc_rollout_dense.batch: ([9 arrays], nlt [2S, n] | None, th, nlt AoS)"""
    th, nlt = rd.batch(I, H, S, n, seed=seed, with_nlt=with_nlt)
    return [dense.soa(th[k], n) for k in NAMES], (None if nlt is None else dense.soa(nlt, n)), th, nlt


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _composed(s, I, H, S, ins, nlt, device, tol, rounds, **over):
    """The polished loop written from the public entries: solve_batch_general carrying controls and v,
    polish_batch_general on the sequence, then the plant update and the target shift in numpy in the step kernel's
    operation order.  Returns numpy arrays: controls, states, sequences, status, res_in, res_out, iters, c, v."""
    n = ins[0].shape[1]
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)) if device else (lambda a: np.ascontiguousarray(a))
    model = [up(a) for a in ins[:7]]
    A, B, Cc = ins[0], ins[1], ins[2]
    x, T = ins[7].copy(), ins[8].copy()
    c, v = up(np.zeros((H * I, n))), up(np.zeros((H * I, n)))
    out = [[] for _ in range(7)]
    for k in range(S):
        _, it = s.solve_batch_general(*model, up(x), up(T), controls=c, v_state=v, inputs=I, want_iters=True, **over)
        _, st, ri, ro = s.polish_batch_general(*model, up(x), up(T), c, tol=tol, max_rounds=rounds, inputs=I)
        u = _np(c).copy()
        bu0, bu1 = B[0] * u[0], B[I] * u[0]
        if I == 2:
            bu0, bu1 = bu0 + B[1] * u[1], bu1 + B[3] * u[1]
        n0 = ((A[0] * x[0] + A[1] * x[1]) + bu0) + Cc[0]
        n1 = ((A[2] * x[0] + A[3] * x[1]) + bu1) + Cc[1]
        x = np.stack([n0, n1])
        T[:-2] = T[2:].copy()
        if nlt is not None and k + 1 < S:
            T[-2:] = nlt[2 * (k + 1):2 * (k + 1) + 2]
        for lst, val in zip(out, (u[:I], x, u, _np(st), _np(ri), _np(ro), _np(it))):
            lst.append(np.array(val))
    cat = lambda l: np.ascontiguousarray(np.concatenate([a.reshape(-1, n) for a in l]))
    return [cat(l) for l in out] + [_np(c).copy(), _np(v).copy()]


def _fused(s, I, H, S, ins, nlt, device, tol, rounds, **over):
    n = ins[0].shape[1]
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)) if device else (lambda a: np.ascontiguousarray(a))
    c, v = up(np.zeros((H * I, n))), up(np.zeros((H * I, n)))
    ri, ro = up(np.zeros((S, n))), up(np.zeros((S, n)))
    cu, cx, sq, st, it = s.rollout_polished(S, *[up(a) for a in ins], None if nlt is None else up(nlt), controls=c,
                                            v_state=v, inputs=I, tol=tol, max_rounds=rounds, want_iters=True,
                                            residuals=(ri, ro), **over)
    if device:
        torch.cuda.synchronize()
    return [np.ascontiguousarray(_np(a)) for a in (cu, cx, sq, st, ri, ro, it, c, v)], s.last_flags


FIELDS = ("controls", "states", "sequences", "status", "residual_in", "residual_out", "iters", "controls_inout",
          "v_inout")


@pytest.mark.parametrize("algo", ["lane", "group"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("with_nlt", [True, False], ids=["nlt", "nonlt"])
@pytest.mark.parametrize("H", [4, 10, 20, 40])
@pytest.mark.parametrize("I", [1, 2])
def test_fused_equals_composed_bits(I, H, with_nlt, device, algo):
    """Nothing is skipped here: unpolished pairs (status -1) are compared like the others.  (At H = 4 there are no
    GROUP kernels of the general form: the request falls to the LANE family in both loops alike.)"""
    S, n = 4, 130
    ins, nlt, _, _ = _case(I, H, S, n, seed=H + I, with_nlt=with_nlt)
    with MpcSolver(horizon=H, device=0, algo=algo) as s:
        want = _composed(s, I, H, S, ins, nlt, device, TOL, ROUNDS)
        got, flags = _fused(s, I, H, S, ins, nlt, device, TOL, ROUNDS)
    st = want[3]
    print(f"I={I} H={H}: unpolished pairs {int((st < 0).sum())}/{st.size}, rounds up to {int(st.max())}")
    for name, a, b in zip(FIELDS, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), name
    assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((st < 0).any())
    assert (st >= 0).any() and np.all(want[5][st >= 0] <= TOL)
    assert got[2].reshape(S, H * I, n)[S - 1].tobytes() == got[7].tobytes()     # controls out = the last sequence


def test_fused_against_composed_with_auto():
    """With algo "auto" the closed loop and the single solve may pick different kernel families (their batches are
    the same size but the entries have their own crossovers), so the sequences are compared to the polish tolerance,
    not bit for bit, and on the first step only, where both solve the same problem: both are KKT points of a QP whose
    Hessian is at least min(R) on the free set, so each is within sqrt(H I) tol / min(R) of the minimiser."""
    I, H, S, n = 2, 10, 4, 130
    ins, nlt, _, _ = _case(I, H, S, n, seed=8)     # CPU checker: 1 of 520 pairs unpolished, none in the first step
    with MpcSolver(horizon=H, device=0) as s:
        want = _composed(s, I, H, S, ins, nlt, True, TOL, ROUNDS)
        got, _ = _fused(s, I, H, S, ins, nlt, True, TOL, ROUNDS)
    both = (want[3][0] >= 0) & (got[3][0] >= 0)
    assert both.mean() >= 1 - CAP
    bound = 2 * np.sqrt(H * I) * TOL / ins[4].min(axis=0)
    err = np.abs(got[2][:H * I] - want[2][:H * I]).max(axis=0)
    print(f"auto: first-step |dU| max {err[both].max():.3e}, whole loop |du0| max "
          f"{np.abs(got[0] - want[0])[:, both].max():.3e}")
    assert np.all(err[both] <= bound[both])


def test_shard_of_a_wider_batch():
    """ld > n through the C entry: a shard's outputs equal the whole batch's columns, padding untouched"""
    I, H, S, n, k0, m = 2, 4, 5, 200, 37, 70
    ins, nlt, _, _ = _case(I, H, S, n, seed=5)
    lib = capi.load_library()
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        (u, x, q, st, ri, ro, it, _, _), _ = _fused(s, I, H, S, ins, nlt, False, TOL, ROUNDS)
        p = s._params()
        sentinel = 777.0
        cu, cx, cq, cri, cro = (np.full((r, n), sentinel) for r in (S * I, 2 * S, S * H * I, S, S))
        cst, cit = np.full((S, n), -7, dtype=np.int32), np.full((S, n), -7, dtype=np.int32)
        off = lambda a: a.ctypes.data + a.itemsize * k0
        io = capi.GeneralIO(inputs=I, n=m, ld=n, A=off(ins[0]), B=off(ins[1]), C=off(ins[2]), Q=off(ins[3]),
                            R=off(ins[4]), lower=off(ins[5]), upper=off(ins[6]), x0=off(ins[7]), targets=off(ins[8]))
        qq = capi.Polish(tol=TOL, max_rounds=ROUNDS, status=off(cst), residual_in=off(cri), residual_out=off(cro))
        flags = C.c_uint32(0)
        rc = lib.tpc_mpc_rollout_polished(s._h, C.byref(p), C.byref(io), S, off(nlt), C.byref(qq), off(cu), off(cx),
                                          off(cit), off(cq), C.byref(flags), capi.HOST, None)
        assert rc == 0
        # the same shard in DEVICE memory, sequences_out and the optional rows left out
        dins = [torch.from_numpy(a).to(DEV) for a in ins]
        du = torch.full((S * I, n), sentinel, dtype=torch.float64, device=DEV)
        doff = lambda t: t.data_ptr() + 8 * k0
        dio = capi.GeneralIO(inputs=I, n=m, ld=n, A=doff(dins[0]), B=doff(dins[1]), C=doff(dins[2]), Q=doff(dins[3]),
                             R=doff(dins[4]), lower=doff(dins[5]), upper=doff(dins[6]), x0=doff(dins[7]),
                             targets=doff(dins[8]))
        dq = capi.Polish(tol=TOL, max_rounds=ROUNDS)
        dnl = torch.from_numpy(nlt).to(DEV)
        rc = lib.tpc_mpc_rollout_polished(s._h, C.byref(p), C.byref(dio), S, doff(dnl), C.byref(dq), doff(du), None,
                                          None, None, C.byref(flags), capi.DEVICE, None)
        assert rc == 0
        torch.cuda.synchronize()
    for got, want, pad in ((cu, u, sentinel), (cx, x, sentinel), (cq, q, sentinel), (cri, ri, sentinel),
                           (cro, ro, sentinel), (cst, st, -7), (cit, it, -7), (du.cpu().numpy(), u, sentinel)):
        assert got[:, k0:k0 + m].tobytes() == np.ascontiguousarray(want[:, k0:k0 + m]).tobytes()
        assert np.all(got[:, :k0] == pad) and np.all(got[:, k0 + m:] == pad)


@pytest.mark.parametrize("kind", ["general", "mixed"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_max_rounds_zero_only_verifies(device, kind):
    """max_rounds = 0 verifies only: controls, states, sequences and iters are rollout_record's bytes, status is 0 or
    -1.  On synth.general_inputs that holds for the whole batch, nothing left out.  mpc_rollout_dense.batch pins input
    1 (lower == upper != 0) in every seventh instance, and dlib's solver never moves a pinned component off its zero
    start: its sequence lies outside the box.  The polish rule begins with u <- clamp(u) (include/tpc_mpc.h), so when
    the clamped sequence verifies (status 0) the clamped one is written -- for those instances "verifies only" still
    changes bytes, in the polished loop as in tpc_mpc_polish_batch_general.  There the comparison takes the instances
    whose recorded sequences lie in the box at every step (measured on the CPU checker: 286 of 300), and the others
    must be exactly the out-of-box ones."""
    I, H, S, n = 2, 10, 6, 300
    if kind == "general":
        from trajectory_controller_amd.synth import general_inputs
        g = general_inputs(H, n, I=I, seed=5)
        ins = [dense.soa(g[k], n) for k in NAMES]
        nlt = np.ascontiguousarray(np.repeat(ins[8][-2:], S, axis=0)
                                   + 0.05 * np.random.default_rng(11).standard_normal((2 * S, n)))
    else:
        ins, nlt, _, _ = _case(I, H, S, n, seed=2)
    up = (lambda a: torch.from_numpy(a).to(DEV)) if device else (lambda a: a)
    with MpcSolver(horizon=H, device=0) as s:
        u, x, q, it = (_np(a) for a in s.rollout_record(S, *[up(a) for a in ins], up(nlt), inputs=I, want_iters=True))
        (pu, px, pq, st, ri, ro, pit, _, _), flags = _fused(s, I, H, S, ins, nlt, device, TOL, 0)
    seqs = q.reshape(S, H, I, n)
    inbox = ((seqs >= ins[5][None, None]) & (seqs <= ins[6][None, None])).all(axis=(0, 1, 2))
    print(f"{kind}: recorded sequences in the box for {int(inbox.sum())}/{n} instances, status 0 in "
          f"{int((st == 0).sum())}/{st.size} pairs")
    if kind == "general":
        assert inbox.all()
    else:
        assert inbox.sum() >= 0.9 * n
        changed = (pq != q).any(axis=0)
        assert not (changed & inbox).any()
    for a, b in ((u, pu), (x, px), (q, pq), (it, pit)):
        assert np.ascontiguousarray(a[:, inbox]).tobytes() == np.ascontiguousarray(b[:, inbox]).tobytes()
    assert np.all((st == 0) | (st == -1)) and (st == -1).any()
    assert np.array_equal(ri, ro) and np.all(ri[st == 0] <= TOL) and np.all(ri[st == -1] > TOL)
    assert flags & capi.FLAG_NOT_POLISHED


def test_existing_entries_untouched_by_a_polished_call():
    """rollout and rollout_record before and after a rollout_polished call on the same handle: the same bytes (the
    polished loop shares the working set, the staging buffer and the gradient workspace)."""
    I, H, S, n = 2, 10, 6, 300
    ins, nlt, _, _ = _case(I, H, S, n, seed=7)
    dins, dnl = [torch.from_numpy(a).to(DEV) for a in ins], torch.from_numpy(nlt).to(DEV)
    with MpcSolver(horizon=H, device=0) as s:
        def both():
            outs = list(s.rollout(S, *ins, nlt, inputs=I, want_iters=True))
            outs += list(s.rollout_record(S, *dins, dnl, inputs=I, want_iters=True))
            g = s.rollout_backward(S, *dins, dnl, sequences=outs[5], states=outs[4], grad_states=torch.ones_like(outs[4]),
                                   inputs=I)
            torch.cuda.synchronize()
            return [_np(a).tobytes() for a in outs] + [_np(g[k]).tobytes() for k in sorted(g)]
        before = both()
        _fused(s, I, H, S, ins, nlt, True, TOL, ROUNDS)
        mid = both()
        _fused(s, I, H, S, ins, nlt, False, TOL, ROUNDS)
        after = both()
    assert before == mid == after


@pytest.mark.parametrize("I,H,S,n,seed,with_nlt", CASES)
def test_every_step_is_the_optimum_on_the_device(I, H, S, n, seed, with_nlt):
    """The GPU's polished sequences fed to the dense closed loop reproduce the GPU's controls and states within the
    bound measured on the CPU checker (tests/test_rollout_polish_host.py, the same inputs); instances with an
    unpolished step are left out, under the 1 % cap.  CPU checker on these inputs: 0/320, 0/400, 1/240, 0/240
    unpolished pairs."""
    ins, nl, th, nlt = _case(I, H, S, n, seed, with_nlt)
    with MpcSolver(horizon=H, device=0) as s:
        (u, x, q, st, *_), flags = _fused(s, I, H, S, ins, nl, True, TOL, ROUNDS)
    assert flags & ~(capi.FLAG_NOT_POLISHED | capi.FLAG_MAX_ITER) == 0
    assert (st < 0).mean() <= CAP, float((st < 0).mean())
    aos = lambda a, r: np.ascontiguousarray(a.T).reshape((n, S) + r)
    u0s, xs, sq = aos(u, (I,)), aos(x, (2,)), aos(q, (H, I))
    dev = rp.deviation_from_optimum(I, H, S, th, nlt, u0s, xs, sq)
    whole = (st >= 0).all(axis=0)
    print(f"I={I} H={H} S={S}: unpolished pairs {int((st < 0).sum())}/{st.size}, largest deviation "
          f"{dev[whole].max():.3e} (bound {BOUND:.3e})")
    assert dev[whole].max() <= BOUND


# ---- autograd ------------------------------------------------------------------------------------------------------

def _loss_grads(I, S, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, S, I)), rng.standard_normal((n, S, 2))


@pytest.mark.parametrize("I,H,S,with_nlt", [(2, 10, 12, True), (1, 20, 6, False), (2, 4, 25, True)])
def test_autograd_matches_dense_reference_at_default_eps(I, H, S, with_nlt):
    """mpc_rollout(polish=True) at the solver's default eps 0.01 against mpc_rollout_dense.closed_loop on the same
    active sets (those of the GPU's polished sequences), at the tolerance
    tests/test_rollout_grad_gpu.py::test_kernel_matches_dense_reference uses.  CPU checker on these inputs: no
    unpolished pair (0/72, 0/36, 0/150)."""
    n = 6
    ins, nl, th, nlt = _case(I, H, S, n, 0, with_nlt)
    G_u, G_x = _loss_grads(I, S, n, 5)
    t = lambda a: torch.from_numpy(dense.soa(a, n)).to(DEV)
    with MpcSolver(horizon=H, device=0) as s:
        assert s.params.eps == 0.01
        leaves = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in ins]
        lnl = None if nl is None else torch.from_numpy(nl).to(DEV).requires_grad_(True)
        u, x = mpc_rollout(s, S, *leaves, new_last_targets=lnl, polish=True)
        L = (u * t(G_u)).sum() + (x * t(G_x)).sum()
        grads = torch.autograd.grad(L, leaves + ([lnl] if with_nlt else []))
        (pu, px, pq, st, *_), _ = _fused(s, I, H, S, ins, nl, True, TOL, ROUNDS)
    assert u.detach().cpu().numpy().tobytes() == pu.tobytes() and x.detach().cpu().numpy().tobytes() == px.tobytes()
    assert (st < 0).mean() <= CAP
    sq = np.ascontiguousarray(pq.T).reshape(n, S, H, I)
    checked = 0
    for i in np.flatnonzero((st >= 0).all(axis=0)):
        ref, _, _, _ = rd.closed_loop(I, H, S, {k: th[k][i] for k in NAMES}, None if nlt is None else nlt[i], sq[i],
                                      G_u[i], G_x[i])
        for j, k in enumerate(list(NAMES) + (["nlt"] if with_nlt else [])):
            got = grads[j][:, i].cpu().numpy()
            want = ref[k].ravel()
            assert np.linalg.norm(got - want) <= 1e-9 * np.linalg.norm(want) + 1e-12, (i, k)
        checked += 1
    assert checked >= n - 1


def test_autograd_matches_finite_differences_of_the_polished_loop():
    I, H, S, n = 2, 10, 8, 6
    ins, nl, _, _ = _case(I, H, S, n, 1)
    G_u, G_x = (torch.from_numpy(dense.soa(a, n)).to(DEV) for a in _loss_grads(I, S, n, 3))
    # The polished loop is the exact one up to tol: a loss evaluation is off by about |G| tol / min(R), a central
    # difference with step h by that over h.  tol = 1e-12 and h = 1e-6 keep tol / h = 1e-6 two orders under the
    # asserted 1e-4 (with the default tol 1e-9 it would be 1e-3, over it).  The CPU checker polishes every pair of
    # these inputs at tol 1e-12 (largest residual out 6.5e-14).
    tol, h = 1e-12, 1e-6
    with MpcSolver(horizon=H, device=0) as s:
        leaves = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in ins]
        lnl = torch.from_numpy(nl).to(DEV).requires_grad_(True)
        u, x = mpc_rollout(s, S, *leaves, new_last_targets=lnl, polish=(tol, ROUNDS))
        grads = torch.autograd.grad((u * G_u).sum() + (x * G_x).sum(), leaves + [lnl])

        def loss(vals):
            u, x, _, st, _ = s.rollout_polished(S, *vals[:9], vals[9], inputs=I, tol=tol, max_rounds=ROUNDS)
            return ((u * G_u).sum(dim=0) + (x * G_x).sum(dim=0)).cpu().numpy(), (st >= 0).all(dim=0).cpu().numpy()
        base = [a.detach() for a in leaves] + [lnl.detach()]
        checked = 0
        for idx, name in ((3, "Q"), (4, "R"), (7, "x0")):
            for r in range(base[idx].shape[0]):
                vp, vm = [b.clone() for b in base], [b.clone() for b in base]
                vp[idx][r] += h
                vm[idx][r] -= h
                (lp, okp), (lm, okm) = loss(vp), loss(vm)
                fd = (lp - lm) / (2 * h)
                got = grads[idx][r].cpu().numpy()
                ok = np.abs(fd - got) <= 1e-4 * np.maximum(1.0, np.abs(got))
                use = okp & okm
                if name == "Q":   # a zero Q is the edge of the model's domain: a step below it breaks min(Q) >= 0
                    use = use & (base[idx][r].cpu().numpy() != 0.0)
                assert use.sum() == 0 or ok[use].mean() >= 0.8, (name, r, fd, got)   # an active set may move
                checked += int(ok[use].sum())
        assert checked >= 20, checked


def test_polish_false_gives_the_unpolished_bytes():
    I, H, S, n = 2, 10, 6, 64
    ins, nl, _, _ = _case(I, H, S, n, 2)
    dins, dnl = [torch.from_numpy(a).to(DEV) for a in ins], torch.from_numpy(nl).to(DEV)
    with MpcSolver(horizon=H, device=0) as s:
        u0, x0, _, _ = s.rollout_record(S, *dins, dnl, inputs=I)
        u1, x1 = mpc_rollout(s, S, *dins, new_last_targets=dnl)
        u2, x2 = mpc_rollout(s, S, *dins, new_last_targets=dnl, polish=False)
        u3, x3 = mpc_rollout(s, S, *dins, new_last_targets=dnl, polish=True)
        torch.cuda.synchronize()
    for a, b in ((u1, u0), (x1, x0), (u2, u0), (x2, x0)):
        assert _np(a).tobytes() == _np(b).tobytes()
    assert _np(u3).tobytes() != _np(u0).tobytes()


def test_closed_loop_weight_fitting_with_polish_lowers_the_loss():
    """The README's fitting loop at the solver's default eps with polish=True: a few Adam steps on log Q and log R of
    a closed loop towards a recorded trajectory lower the loss"""
    I, H, S, n = 2, 10, 10, 64
    ins, nl, _, _ = _case(I, H, S, n, 4)
    ins, nlt = [torch.from_numpy(a).to(DEV) for a in ins], torch.from_numpy(nl).to(DEV)
    with MpcSolver(horizon=H, device=0) as s:
        with torch.no_grad():
            u_goal, x_goal = mpc_rollout(s, S, *ins, new_last_targets=nlt, polish=True)
        logq = torch.log(ins[3] * 3.0 + 1e-3).clone().requires_grad_(True)
        logr = torch.log(ins[4] * 0.3).clone().requires_grad_(True)
        opt = torch.optim.Adam([logq, logr], lr=0.1)
        losses = []
        for _ in range(6):
            opt.zero_grad()
            u, x = mpc_rollout(s, S, *ins[:3], torch.exp(logq), torch.exp(logr), *ins[5:], new_last_targets=nlt,
                               polish=True)
            loss = ((x - x_goal) ** 2).sum() + ((u - u_goal) ** 2).sum()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# ---- flags ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what,flag", [("nan", capi.FLAG_NONFINITE), ("R", capi.FLAG_BAD_MODEL),
                                       ("bounds", capi.FLAG_BAD_MODEL)])
def test_flagged_instances_behave_as_in_the_rollout(what, flag):
    I, H, S, n, bad = 2, 10, 5, 96, 17
    ins, nl, _, _ = _case(I, H, S, n, 1)       # CPU checker: 1 of 480 pairs of the clean batch unpolished
    if what == "nan":
        ins[7][1, bad] = np.nan                # the state: it stays non-finite through the plant, so every step is
    elif what == "R":
        ins[4][1, bad] = 0.0
    else:
        ins[6][0, bad] = ins[5][0, bad] - 0.1
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        u, x, q, it = s.rollout_record(S, *ins, nl, inputs=I, want_iters=True)
        rflags = s.last_flags
        (pu, px, pq, st, ri, ro, pit, _, _), flags = _fused(s, I, H, S, ins, nl, False, TOL, ROUNDS)
    others = np.arange(n) != bad
    # the instance's rows are the rollout's, bit for bit; its status is -1 and its residuals 0 in every step
    for a, b in ((u, pu), (x, px), (q, pq), (it, pit)):
        assert np.ascontiguousarray(a[:, bad]).tobytes() == np.ascontiguousarray(b[:, bad]).tobytes()
    assert np.all(st[:, bad] == -1) and np.all(ri[:, bad] == 0.0) and np.all(ro[:, bad] == 0.0)
    # ... it raises the rollout's flags, and not NOT_POLISHED on its own
    print(f"{what}: rollout flags {rflags:#x}, polished rollout flags {flags:#x}")
    assert flags & flag and (rflags & ~capi.FLAG_MAX_ITER) & ~flags == 0
    assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((st[:, others] < 0).any())
    assert (st[:, others] >= 0).mean() >= 1 - CAP


# ---- full size -----------------------------------------------------------------------------------------------------

FULL = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd.synth import general_inputs
H, n, S, I = 20, 262144, 10, 2
g = general_inputs(H, n, I=I, seed=5)
names = ["A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets"]
ins = [torch.from_numpy(np.ascontiguousarray(g[k].reshape(n, -1).T)).to("cuda:0") for k in names]
with MpcSolver(horizon=H, device=0) as s:
    u, x, q, st, _ = s.rollout_polished(S, *ins, inputs=I)
    torch.cuda.synchronize()
    flags = s.last_flags
share = float((st >= 0).double().mean())
print("flags", flags, "polished share", share, "finite", bool(torch.isfinite(u).all() and torch.isfinite(x).all()))
assert flags & ~(capi.FLAG_MAX_ITER | capi.FLAG_NOT_POLISHED) == 0
assert share >= 0.99 and torch.isfinite(u).all() and torch.isfinite(x).all()
"""


def test_full_size_run():
    """262 144 x N = 20 x 10 steps, two inputs, DEVICE memory, once, in a child process under its own time limit
    (synth.general_inputs, seed 5: the CPU checker polishes 3000 of 3000 pairs of the first 300 instances)."""
    r = subprocess.run([sys.executable, "-c", FULL, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
