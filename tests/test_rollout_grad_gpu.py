"""GPU tests of the closed-loop backward: the recording forward (tpc_mpc_rollout_record) changes nothing of the
rollout, the gfx950 kernel of tpc_mpc_rollout_backward equals the host path bit for bit and the dense reference,
and trajectory_controller_amd.mpc_rollout matches finite differences of the GPU rollout."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.test_rollout_grad_host import KEY, NAMES, _loss_grads, _reference_batch, _soa_inputs
from trajectory_controller_amd import MpcSolver, capi, mpc_rollout
from trajectory_controller_amd.synth import general_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _general(I, H, n, seed=0):
    g = general_inputs(H, n, I=I, seed=seed)
    ins = [np.ascontiguousarray(g[k].reshape(n, -1).T) for k in NAMES]
    rng = np.random.default_rng(seed + 17)
    return ins, rng


def _nlt(ins, H, S, n, rng):
    last = ins[8][2 * (H - 1):2 * H]
    return np.ascontiguousarray(np.repeat(last, S, axis=0) + 0.05 * rng.standard_normal((2 * S, n)))


@pytest.mark.parametrize("algo", ["auto", "lane", "group"])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_rollout_record_changes_nothing(algo, mem):
    I, H, S, n = 2, 10, 6, 300
    ins, rng = _general(I, H, n, seed=3)
    nlt = _nlt(ins, H, S, n, rng)
    with MpcSolver(horizon=H, device=0, algo=algo) as s:
        if mem == "device":
            args = [torch.from_numpy(a).to(DEV) for a in ins]
            nl = torch.from_numpy(nlt).to(DEV)
            c1 = torch.zeros(H * I, n, dtype=torch.float64, device=DEV)
            c2 = c1.clone()
        else:
            args, nl = ins, nlt
            c1 = np.zeros((H * I, n))
            c2 = c1.copy()
        u, x, it = s.rollout(S, *args, nl, controls=c1, inputs=I, want_iters=True)
        u2, x2, q, it2 = s.rollout_record(S, *args, nl, controls=c2, inputs=I, want_iters=True)
        torch.cuda.synchronize()
    cv = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a
    u, x, it, u2, x2, q, it2, c1, c2 = map(cv, (u, x, it, u2, x2, q, it2, c1, c2))
    assert u.tobytes() == u2.tobytes() and x.tobytes() == x2.tobytes() and np.array_equal(it, it2)
    assert c1.tobytes() == c2.tobytes()
    q = q.reshape(S, H * I, n)
    for k in range(S):
        assert q[k, :I].tobytes() == u[k * I:(k + 1) * I].tobytes()
    assert q[S - 1].tobytes() == c2.tobytes()


def test_rollout_record_shard_of_a_wider_batch():
    """ld > n through the C entry: a shard's outputs equal the whole batch's columns, padding untouched"""
    I, H, S, n, k0, m = 2, 4, 5, 200, 37, 70
    ins, rng = _general(I, H, n, seed=5)
    nlt = _nlt(ins, H, S, n, rng)
    lib = capi.load_library()
    with MpcSolver(horizon=H, device=0) as s:
        u, x, q, _ = s.rollout_record(S, *ins, nlt, inputs=I)
        p = s._params()
        sentinel = 777.0
        cu, cx, cq = (np.full((r, n), sentinel) for r in (S * I, 2 * S, S * H * I))
        off = lambda a: None if a is None else a.ctypes.data + 8 * k0
        io = capi.GeneralIO(inputs=I, n=m, ld=n, A=off(ins[0]), B=off(ins[1]), C=off(ins[2]), Q=off(ins[3]),
                            R=off(ins[4]), lower=off(ins[5]), upper=off(ins[6]), x0=off(ins[7]), targets=off(ins[8]))
        flags = C.c_uint32(0)
        rc = lib.tpc_mpc_rollout_record(s._h, C.byref(p), C.byref(io), S, off(nlt), off(cu), off(cx), None, off(cq),
                                        C.byref(flags), capi.HOST, None)
        assert rc == 0
    for got, want in ((cu, u), (cx, x), (cq, q)):
        assert got[:, k0:k0 + m].tobytes() == np.ascontiguousarray(want[:, k0:k0 + m]).tobytes()
        assert np.all(got[:, :k0] == sentinel) and np.all(got[:, k0 + m:] == sentinel)


def _recorded(I, H, S, n, seed, flag_at=()):
    """inputs, nlt, sequences, states, G_u, G_x of a device rollout_record (numpy); instances in flag_at get a NaN
    in their dL/dstates"""
    ins, rng = _general(I, H, n, seed=seed)
    nlt = _nlt(ins, H, S, n, rng)
    with MpcSolver(horizon=H, device=0) as s:
        _, x, q, _ = s.rollout_record(S, *[torch.from_numpy(a).to(DEV) for a in ins], torch.from_numpy(nlt).to(DEV),
                                      inputs=I)
        torch.cuda.synchronize()
        x, q = x.cpu().numpy(), q.cpu().numpy()
    G_u = rng.standard_normal((S * I, n))
    G_x = rng.standard_normal((2 * S, n))
    for i in flag_at:
        if i < n:
            G_x[1, i] = np.nan
    return ins, nlt, q, x, G_u, G_x


@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H,S", [(4, 20), (20, 7), (40, 3)])
@pytest.mark.parametrize("n", [1, 63, 64, 4097])
def test_kernel_equals_host_path_bits(I, H, S, n):
    flag_at = (n // 2, 33) if n > 1 else ()
    ins, nlt, q, x, G_u, G_x = _recorded(I, H, S, n, seed=H + S + I, flag_at=flag_at)
    g = dict(sequences=q, states=x, grad_controls=G_u, grad_states=G_x)
    with MpcSolver(horizon=H, device=None) as s:
        host = s.rollout_backward(S, *ins, nlt, inputs=I, **g)
        hflags = s.last_flags
    with MpcSolver(horizon=H, device=0) as s:
        dev = s.rollout_backward(S, *[torch.from_numpy(a).to(DEV) for a in ins], torch.from_numpy(nlt).to(DEV),
                                 inputs=I, **{k: torch.from_numpy(v).to(DEV) for k, v in g.items()})
        dflags = s.last_flags
        torch.cuda.synchronize()
    assert hflags == dflags == (capi.FLAG_NONFINITE if flag_at else 0)
    for k, a in host.items():
        b = dev[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), k
    for i in flag_at:
        assert all(np.all(host[k][..., i] == 0.0) for k in host)


@pytest.mark.parametrize("I,H,S,with_nlt", [(2, 10, 12, True), (1, 20, 6, False), (2, 4, 25, True)])
def test_kernel_matches_dense_reference(I, H, S, with_nlt):
    """HOST memory on the default stream and DEVICE memory on a side stream, against the dense closed loop"""
    n = 6
    th, nlt, G_u, G_x, refs, seqs, states, keep, _ = _reference_batch(I, H, S, n, with_nlt)
    ins, nl, g = _soa_inputs(I, H, S, th, nlt, G_u, G_x, seqs, states, n)
    with MpcSolver(horizon=H, device=0) as s:
        host = s.rollout_backward(S, *ins, nl, inputs=I, **g)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            dv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
            dev = s.rollout_backward(S, *[dv(a) for a in ins], dv(nl), inputs=I, **{k: dv(v) for k, v in g.items()})
        side.synchronize()
    for out in (host, {k: v.cpu().numpy() for k, v in dev.items()}):
        for i in np.flatnonzero(keep):
            for k in list(NAMES) + (["nlt"] if with_nlt else []):
                got = out["new_last_targets" if k == "nlt" else KEY[k]][:, i]
                want = refs[i][k].ravel()
                assert np.linalg.norm(got - want) <= 1e-9 * np.linalg.norm(want) + 1e-12, (i, k)
    assert host["A"].tobytes() == dev["A"].cpu().numpy().tobytes()


def _device_case(I, H, S, n, seed=1):
    th, nlt = rd.batch(I, H, S, n, seed=seed)
    t = lambda a: torch.from_numpy(dense.soa(a, n)).to(DEV)
    return [t(th[k]) for k in NAMES], t(nlt)


def test_autograd_matches_finite_differences():
    I, H, S, n = 2, 10, 8, 6
    ins, nlt = _device_case(I, H, S, n)
    G_u, G_x = (torch.from_numpy(np.ascontiguousarray(a.reshape(n, -1).T)).to(DEV) for a in _loss_grads(I, S, n, 3))
    over = dict(eps=1e-10, max_iter=200000)
    with MpcSolver(horizon=H, device=0) as s:
        leaves = [a.clone().requires_grad_(True) for a in ins] + [nlt.clone().requires_grad_(True)]
        u, x = mpc_rollout(s, S, *leaves[:9], new_last_targets=leaves[9], **over)
        L = (u * G_u).sum() + (x * G_x).sum()
        grads = torch.autograd.grad(L, leaves)

        def loss(vals):
            u, x, _ = s.rollout(S, *vals[:9], vals[9], inputs=I, **over)
            return ((u * G_u).sum(dim=0) + (x * G_x).sum(dim=0)).cpu().numpy()   # per instance
        base = [a.detach() for a in leaves]
        checked = 0
        for idx, name in ((3, "Q"), (4, "R"), (1, "B"), (7, "x0"), (8, "targets"), (9, "nlt")):
            rows = range(2, base[idx].shape[0]) if name == "nlt" else range(base[idx].shape[0])
            for r in list(rows)[:4]:
                h = 1e-6
                vp = [b.clone() for b in base]
                vm = [b.clone() for b in base]
                vp[idx][r] += h
                vm[idx][r] -= h
                fd = (loss(vp) - loss(vm)) / (2 * h)
                got = grads[idx][r].cpu().numpy()
                ok = np.abs(fd - got) <= 1e-4 * np.maximum(1.0, np.abs(got))
                if name == "Q":   # a zero Q is the edge of the model's domain: a step below it breaks min(Q) >= 0
                    ok = ok[base[idx][r].cpu().numpy() != 0.0]
                assert ok.mean() >= 0.8, (name, r, fd, got)   # an instance whose active set moves may differ
                checked += int(ok.sum())
        assert checked > 50


def test_closed_loop_weight_fitting_lowers_the_loss():
    """A few Adam steps on log Q and log R of a closed loop towards a recorded trajectory lower the loss"""
    I, H, S, n = 2, 10, 10, 64
    ins, nlt = _device_case(I, H, S, n, seed=4)
    with MpcSolver(horizon=H, device=0) as s:
        with torch.no_grad():
            u_goal, x_goal = mpc_rollout(s, S, *ins, new_last_targets=nlt, eps=1e-8)
        logq = torch.log(ins[3] * 3.0 + 1e-3).clone().requires_grad_(True)
        logr = torch.log(ins[4] * 0.3).clone().requires_grad_(True)
        opt = torch.optim.Adam([logq, logr], lr=0.1)
        losses = []
        for _ in range(6):
            opt.zero_grad()
            u, x = mpc_rollout(s, S, *ins[:3], torch.exp(logq), torch.exp(logr), *ins[5:], new_last_targets=nlt,
                               eps=1e-8)
            loss = ((x - x_goal) ** 2).sum() + ((u - u_goal) ** 2).sum()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
