"""CPU tests of the closed loops against a separate plant (tpc_mpc_rollout_plant, _plant_backward, _plant_forward;
MpcSolver's plant= / disturbance= keywords) on a host-only handle: the Newton loop against its definition composed from
the public polish entry and the plant line in numpy, the parents' bits when the plant is the controller's model, the
transpose identity of the forward and backward entries with the plant's and the disturbance's terms, and the entries'
argument checks and flags.

The mismatched plant is Ap = A o (1 + s N), Bp = B o (1 + s N), Cp = C + s N, d = 0.1 s N with standard normal N and
s = PLANT_SCALE, the largest of 0.2, 0.1, 0.05, 0.02 for which the composed definition below (the parent's code only)
leaves at most 10 % of synth.general_inputs seed 5 unverified on every shape; the shares are printed by
test_plant_scale_keeps_the_unverified_share_under_the_cap and quoted in DESIGN.md section 18."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_rollout_newton_host import COVERAGE_CAP, N, ROUNDS, SHAPES, TOL, inputs, newton_host, soa_inputs
from tests.test_rollout_tangent_host import BOUND as IDENTITY_BOUND, CASES, mismatch, recorded_case
from tests.model import mpc_rollout_tangent_dense as td
from trajectory_controller_amd import MpcSolver, capi

PLANT_SCALE = 0.05


def make_plant(ins, I, S, scale=PLANT_SCALE, seed=3):
    """((Ap, Bp, Cp), disturbance [2S, n]) around the controller's model ins[0..2]"""
    rng = np.random.default_rng(seed)
    n = ins[0].shape[1]
    Ap = ins[0] * (1.0 + scale * rng.standard_normal((4, n)))
    Bp = ins[1] * (1.0 + scale * rng.standard_normal((2 * I, n)))
    Cp = ins[2] + scale * rng.standard_normal((2, n))
    return (Ap, Bp, Cp), 0.1 * scale * rng.standard_normal((2 * S, n))


def composed_plant(I, H, S, ins, nlt, plant, dist, tol=TOL, rounds=ROUNDS):
    """tests/test_rollout_newton_host.py::composed with the plant line: the shift, polish_batch_general with the
    controller's model, then x <- ((Ap x + Bp u0) + Cp) (+ d_k) in the tail's order"""
    n = ins[0].shape[1]
    model = ins[:7]
    A, B, Cc = plant if plant is not None else ins[:3]
    x, T, c = ins[7].copy(), ins[8].copy(), np.zeros((H * I, n))
    alive, first = np.ones(n, dtype=bool), np.full(n, S, dtype=np.int32)
    u, xs, sq = np.zeros((S * I, n)), np.zeros((S * 2, n)), np.zeros((S * H * I, n))
    st, ri, ro = np.full((S, n), -1, dtype=np.int32), np.zeros((S, n)), np.zeros((S, n))
    with MpcSolver(horizon=H, device=None) as s, np.errstate(all="ignore"):
        for k in range(S):
            c[:-I] = c[I:].copy()
            _, st_k, ri_k, ro_k = s.polish_batch_general(*model, x, T, c, tol=tol, max_rounds=rounds, inputs=I)
            ok = alive & (st_k >= 0)
            first[alive & ~ok] = k
            alive = ok
            u0 = c[:I]
            xn = np.empty((2, n))
            for r in range(2):
                bu = B[r * I] * u0[0]
                if I == 2:
                    bu = bu + B[r * I + 1] * u0[1]
                xn[r] = ((A[2 * r] * x[0] + A[2 * r + 1] * x[1]) + bu) + Cc[r]
                if dist is not None:
                    xn[r] = xn[r] + dist[2 * k + r]
            x = xn
            u[k * I:(k + 1) * I, ok], xs[2 * k:2 * k + 2, ok] = u0[:, ok], x[:, ok]
            sq[k * H * I:(k + 1) * H * I, ok] = c[:, ok]
            st[k, ok], ri[k, ok], ro[k, ok] = st_k[ok], ri_k[ok], ro_k[ok]
            T[:-2] = T[2:].copy()
            if nlt is not None and k + 1 < S:
                T[-2:] = nlt[2 * (k + 1):2 * (k + 1) + 2]
    c[:, ~alive] = 0.0
    return u, xs, sq, st, first, ri, ro, c


def plant_newton(I, H, S, ins, nlt, plant, dist, controls=None):
    n = ins[0].shape[1]
    ri, ro = np.full((S, n), 7.0), np.full((S, n), 7.0)
    with MpcSolver(horizon=H, device=None) as s:
        u, x, q, st, it, first = s.rollout_newton(S, *ins, nlt, controls=controls, inputs=I, tol=TOL, max_rounds=ROUNDS,
                                                  fallback="none", want_iters=True, residuals=(ri, ro), plant=plant,
                                                  disturbance=dist)
        return u, x, q, st, it, first, ri, ro, s.last_flags


@functools.lru_cache(maxsize=None)
def case(I, H, S, with_nlt, kind="general"):
    th, nlt = inputs(kind, I, H, S, with_nlt=with_nlt)
    ins, nl = soa_inputs(th, nlt, N)
    return ins, nl, make_plant(ins, I, S)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_symbols_and_abi_version():
    lib = capi.load_library()
    for name in ("tpc_mpc_rollout_plant", "tpc_mpc_rollout_plant_backward", "tpc_mpc_rollout_plant_forward"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.tpc_mpc_abi_version() == 5 == capi.ABI_VERSION


def test_plant_scale_keeps_the_unverified_share_under_the_cap():
    for I, H, S in SHAPES:
        ins, nl, (plant, dist) = case(I, H, S, True)
        first = composed_plant(I, H, S, ins, nl, plant, dist)[4]
        share = float(np.mean(first < S))
        print(f"I={I} H={H} S={S}: unverified share {share:.3f} at s = {PLANT_SCALE}")
        assert share <= COVERAGE_CAP


# ---- 1. the definition, bit for bit ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["plant", "disturbance", "both"])
@pytest.mark.parametrize("with_nlt", [True, False], ids=["nlt", "nonlt"])
@pytest.mark.parametrize("I,H,S", SHAPES)
def test_newton_loop_equals_its_definition_bit_for_bit(I, H, S, with_nlt, mode):
    ins, nl, (plant, dist) = case(I, H, S, with_nlt)
    plant = plant if mode != "disturbance" else None
    dist = dist if mode != "plant" else None
    ctrl = np.zeros((H * I, N))
    u, x, q, st, it, first, ri, ro, flags = plant_newton(I, H, S, ins, nl, plant, dist, controls=ctrl)
    wu, wx, wq, wst, wfirst, wri, wro, wc = composed_plant(I, H, S, ins, nl, plant, dist)
    for got, want, what in ((u, wu, "controls"), (x, wx, "states"), (q, wq, "sequences"), (st, wst, "status"),
                            (first, wfirst, "first_unverified"), (ri, wri, "residual_in"), (ro, wro, "residual_out"),
                            (ctrl, wc, "controls_inout")):
        assert same_bits(got, want), what
    assert (flags == capi.FLAG_NOT_POLISHED) == bool((first < S).any())
    # the plant matters: the parent's loop gives other states
    parent = newton_host(I, H, S, ins, nl)
    assert not same_bits(parent[1], x)


# ---- 2. the parents' bits --------------------------------------------------------------------------------------------

def _raw_newton_null_plant(I, H, S, ins, nl):
    """tpc_mpc_rollout_plant, TPC_MPC_LOOP_NEWTON, with a plant of all NULLs, through ctypes"""
    lib = capi.load_library()
    n = ins[0].shape[1]
    keep = [np.ascontiguousarray(a) for a in ins]
    u, x, q = np.empty((S * I, n)), np.empty((2 * S, n)), np.empty((S * H * I, n))
    st, it, first = np.empty((S, n), np.int32), np.empty((S, n), np.int32), np.empty(n, np.int32)
    ptr = lambda a: a.ctypes.data
    with MpcSolver(horizon=H, device=None) as s:
        p = s._params()
        io = capi.GeneralIO(inputs=I, n=n, ld=n, **{k: ptr(a) for k, a in zip(
            ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets"), keep)})
        pol = capi.Polish(tol=TOL, max_rounds=ROUNDS, reserved=0, status=ptr(st), residual_in=None, residual_out=None)
        pl, flags = capi.Plant(), C.c_uint32(0)
        rc = lib.tpc_mpc_rollout_plant(s._h, C.byref(p), C.byref(io), C.byref(pl), capi.LOOP_NEWTON, S,
                                       None if nl is None else ptr(nl), C.byref(pol), capi.NEWTON_FALLBACK_NONE, ptr(u),
                                       ptr(x), ptr(it), ptr(q), ptr(first), C.byref(flags), capi.HOST, None)
        assert rc == capi.OK
    return u, x, q, st, it, first, flags.value


@pytest.mark.parametrize("I,H,S", SHAPES)
def test_no_plant_and_a_copy_of_the_model_give_the_parents_bits(I, H, S):
    ins, nl, _ = case(I, H, S, True)
    parent = newton_host(I, H, S, ins, nl)
    null = _raw_newton_null_plant(I, H, S, ins, nl)
    for got, want in zip(null[:6], parent[:6]):
        assert same_bits(got, want)
    assert null[6] == parent[8]
    copies = tuple(a.copy() for a in ins[:3])
    same = plant_newton(I, H, S, ins, nl, copies, None)
    for got, want in zip(same, parent):
        assert same_bits(np.asarray(got), np.asarray(want))
    # the derivative entries at the parent's recorded loop
    u, x, q = parent[:3]
    rng = np.random.default_rng(1)
    G_u, G_x = rng.standard_normal(u.shape), rng.standard_normal(x.shape)
    tan = td.soa_tangents(td.random_tangents(I, H, S, N, 4, K=2), N)
    with MpcSolver(horizon=H, device=None) as s:
        g0 = s.rollout_backward(S, *ins, nl, sequences=q, states=x, grad_controls=G_u, grad_states=G_x, inputs=I)
        g1 = s.rollout_backward(S, *ins, nl, sequences=q, states=x, grad_controls=G_u, grad_states=G_x, inputs=I,
                                plant=copies)
        # no plant arrays, the disturbance's gradient alone: the plant terms stay in dA, dB, dC, bit for bit
        g2 = s.rollout_backward(S, *ins, nl, sequences=q, states=x, grad_controls=G_u, grad_states=G_x, inputs=I,
                                want=tuple(g0) + ("disturbance",))
        t0 = s.rollout_forward(S, *ins, nl, sequences=q, states=x, tangents=tan, inputs=I)
        # the model's tangents given as the plant's too: the same line on the same values
        t1 = s.rollout_forward(S, *ins, nl, sequences=q, states=x, inputs=I, plant=copies,
                               tangents=dict(tan, Ap=tan["A"], Bp=tan["B"], Cp=tan["C"]))
    for k in g0:
        assert same_bits(g2[k], g0[k]), k
        if k in ("A", "B", "C"):
            total = g1[k] + g1[k + "p"]
            assert np.abs(total - g0[k]).max() <= 1e-12 * np.abs(g0[k]).max(), k
        else:
            assert same_bits(g1[k], g0[k]), k
    assert same_bits(g1["disturbance"], g2["disturbance"])
    assert same_bits(t1[0], t0[0]) and same_bits(t1[1], t0[1])


# ---- 3. dA and dAp are different things --------------------------------------------------------------------------------

@pytest.mark.parametrize("I,H,S", SHAPES)
def test_plant_and_controller_gradients_differ_and_split_the_parents(I, H, S):
    ins, nl, (plant, dist) = case(I, H, S, True)
    u, x, q, st, it, first, *_ = plant_newton(I, H, S, ins, nl, plant, dist)
    carried = first == S
    assert carried.mean() >= 1.0 - COVERAGE_CAP
    G_u, G_x = np.ones_like(u), np.ones_like(x)
    with MpcSolver(horizon=H, device=None) as s:
        g = s.rollout_backward(S, *ins, nl, sequences=q, states=x, grad_controls=G_u, grad_states=G_x, inputs=I,
                               plant=plant, disturbance=dist)
        assert s.last_flags == 0
    scale = max(np.abs(g["A"][:, carried]).max(), np.abs(g["Ap"][:, carried]).max())
    assert np.abs(g["A"][:, carried] - g["Ap"][:, carried]).max() > 1e-6 * scale
    # the last step's mu is G_x's last row: nothing follows it
    assert same_bits(g["disturbance"][2 * S - 2:], G_x[2 * S - 2:])


# ---- 4. the transpose identity -----------------------------------------------------------------------------------------

def plant_identity(s, I, H, S, n, with_nlt, K, to=lambda a: a, back=lambda a: a):
    ins, nl, sq, st, *_ = recorded_case(I, H, S, n, with_nlt)
    plant, _ = make_plant(ins, I, S, scale=0.2)
    rng = np.random.default_rng(6)
    G_u, G_x = rng.standard_normal((S * I, n)), rng.standard_normal((2 * S, n))
    tan = td.soa_tangents(td.random_tangents(I, H, S, n, 10, with_nlt=with_nlt, K=K), n)
    tan.update(Ap=rng.standard_normal((K, 4, n)), Bp=rng.standard_normal((K, 2 * I, n)),
               Cp=rng.standard_normal((K, 2, n)), disturbance=rng.standard_normal((K, 2 * S, n)))
    dins, dnl, dplant = [to(a) for a in ins], (None if nl is None else to(nl)), tuple(to(a) for a in plant)
    tu, tx = s.rollout_forward(S, *dins, dnl, sequences=to(sq), states=to(st), inputs=I, plant=dplant,
                               tangents={k: to(v) for k, v in tan.items()})
    assert s.last_flags == 0
    g = s.rollout_backward(S, *dins, dnl, sequences=to(sq), states=to(st), grad_controls=to(G_u), grad_states=to(G_x),
                           inputs=I, plant=dplant)
    assert s.last_flags == 0
    tu, tx, g = back(tu), back(tx), {k: back(v) for k, v in g.items()}
    worst = max(float(mismatch([G_u * tu[d], G_x * tx[d]], [g[k] * tan[k][d] for k in tan]).max()) for d in range(K))
    return worst, (ins, nl, sq, st, plant, tan, tu, tx)


@pytest.mark.parametrize("with_nlt", [True, False], ids=["nlt", "nonlt"])
@pytest.mark.parametrize("I,H,S", CASES)
def test_plant_forward_is_the_transpose_of_plant_backward(I, H, S, with_nlt):
    n, K = 40, 3
    with MpcSolver(horizon=H, device=None) as s:
        worst, (ins, nl, sq, st, plant, tan, tu, tx) = plant_identity(s, I, H, S, n, with_nlt, K)
        print(f"I={I} H={H} S={S} nlt={with_nlt}: largest mismatch {worst:.3e} (bound {IDENTITY_BOUND:.3e})")
        assert worst <= IDENTITY_BOUND, worst
        # K = 3 is three K = 1 calls
        for d in range(K):
            one = s.rollout_forward(S, *ins, nl, sequences=sq, states=st, inputs=I, plant=plant,
                                    tangents={k: np.ascontiguousarray(v[d:d + 1]) for k, v in tan.items()})
            assert same_bits(one[0][0], tu[d]) and same_bits(one[1][0], tx[d])
        # a missing plant tangent is an explicit zero
        part = {k: v for k, v in tan.items() if k not in ("Bp", "disturbance")}
        zeros = dict(part, Bp=np.zeros_like(tan["Bp"]), disturbance=np.zeros_like(tan["disturbance"]))
        a = s.rollout_forward(S, *ins, nl, sequences=sq, states=st, inputs=I, plant=plant, tangents=part)
        b = s.rollout_forward(S, *ins, nl, sequences=sq, states=st, inputs=I, plant=plant, tangents=zeros)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
        # a tangent of the disturbance's row k alone reaches nothing before step k (tstates) / k + 1 (tcontrols)
        k = S // 2
        only = np.zeros((1, 2 * S, n))
        only[0, 2 * k:2 * k + 2] = 1.0
        tu1, tx1 = s.rollout_forward(S, *ins, nl, sequences=sq, states=st, inputs=I, plant=plant,
                                     tangents={"disturbance": only})
        assert not tu1[0][:(k + 1) * I].any() and not tx1[0][:2 * k].any()
        assert same_bits(tx1[0][2 * k:2 * k + 2], only[0, 2 * k:2 * k + 2])


# ---- 6. arguments and flags --------------------------------------------------------------------------------------------

def _status(fn):
    with pytest.raises(capi.TpcMpcError) as e:
        fn()
    return capi.STATUS_NAMES[e.value.status]


def test_argument_checks():
    I, H, S = 2, 10, 4
    ins, nl, ((Ap, Bp, Cp), dist) = case(2, 10, 10, True)
    nl, dist = np.ascontiguousarray(nl[:2 * S]), np.ascontiguousarray(dist[:2 * S])
    lib = capi.load_library()
    with MpcSolver(horizon=H, device=None) as s:
        kw = dict(inputs=I, fallback="none")
        assert _status(lambda: s.rollout_newton(S, *ins, nl, plant=(Ap, None, Cp), **kw)) == "BAD_ARG"
        assert _status(lambda: s.rollout_newton(S, *ins, nl, plant=(None, Bp, None), **kw)) == "BAD_ARG"
        assert _status(lambda: s.rollout_newton(S, *ins, nl, plant=(Ap, Bp, Cp), inputs=I, fallback="solve")) == "NO_DEVICE"
        assert _status(lambda: s.rollout_polished(S, *ins, nl, plant=(Ap, Bp, Cp), inputs=I)) == "NO_DEVICE"
        assert _status(lambda: s.rollout_record(S, *ins, nl, plant=(Ap, Bp, Cp), inputs=I)) == "NO_DEVICE"
        # checked before the device is asked for
        assert _status(lambda: s.rollout_record(S, *ins, nl, plant=(Ap, None, None), inputs=I)) == "BAD_ARG"
        # an unknown loop, fp32, n == 0 and steps == 0 through the C entry
        p, io, pl = s._params(), capi.GeneralIO(inputs=I, n=0, ld=0), capi.Plant()
        pol = capi.Polish(tol=TOL, max_rounds=ROUNDS)
        call = lambda p, io, loop, steps: lib.tpc_mpc_rollout_plant(
            s._h, C.byref(p), C.byref(io), C.byref(pl), loop, steps, None, C.byref(pol), capi.NEWTON_FALLBACK_NONE, None,
            None, None, None, None, None, capi.HOST, None)
        assert call(p, io, capi.LOOP_NEWTON, S) == capi.OK
        assert capi.STATUS_NAMES[call(p, io, 7, S)] == "BAD_ARG"
        io.n = io.ld = N
        assert call(p, io, capi.LOOP_NEWTON, 0) == capi.OK
        p.dtype = capi.F32
        assert capi.STATUS_NAMES[call(p, io, capi.LOOP_NEWTON, S)] == "BAD_ARG"
        p.dtype = capi.F64
        # the plant's gradients / tangents need the plant
        u, x, q, *_ = s.rollout_newton(S, *ins, nl, plant=(Ap, Bp, Cp), disturbance=dist, **kw)
        assert _status(lambda: s.rollout_backward(S, *ins, nl, sequences=q, states=x, inputs=I, want=("Ap",))) == "BAD_ARG"
        assert _status(lambda: s.rollout_forward(S, *ins, nl, sequences=q, states=x, inputs=I,
                                                 tangents={"Ap": np.ones((1, 4, N))})) == "BAD_ARG"


@pytest.mark.parametrize("where", ["Ap", "disturbance"])
def test_a_nan_flags_and_zeroes_exactly_that_instance(where):
    I, H, S = 2, 10, 10
    ins, nl, ((Ap, Bp, Cp), dist) = case(I, H, S, True)
    clean = plant_newton(I, H, S, ins, nl, (Ap, Bp, Cp), dist)
    Ap, dist, bad = Ap.copy(), dist.copy(), 17
    if where == "Ap":
        Ap[2, bad] = np.nan
    else:
        dist[2 * (S - 1) + 1, bad] = np.nan        # the last row: no later step would meet it
    u, x, q, st, it, first, ri, ro, flags = plant_newton(I, H, S, ins, nl, (Ap, Bp, Cp), dist)
    assert flags & capi.FLAG_NONFINITE
    assert first[bad] == 0 and (st[:, bad] == -1).all()
    assert not u[:, bad].any() and not x[:, bad].any() and not q[:, bad].any()
    others = np.arange(N) != bad
    for got, want in zip((u, x, q, st, first), (clean[0], clean[1], clean[2], clean[3], clean[5])):
        assert same_bits(np.ascontiguousarray(got[..., others]), np.ascontiguousarray(want[..., others]))
    # the derivative entries: the plant's NaN zeroes that instance's gradients and tangents
    cu, cx, cq = clean[:3]
    with MpcSolver(horizon=H, device=None) as s:
        if where == "Ap":
            g = s.rollout_backward(S, *ins, nl, sequences=cq, states=cx, grad_states=np.ones_like(cx), inputs=I,
                                   plant=(Ap, Bp, Cp))
            assert s.last_flags & capi.FLAG_NONFINITE
            assert all(not v[..., bad].any() for v in g.values())
            assert g["Ap"][:, others].any()
        else:
            tdist = np.ones((1, 2 * S, N))
            tdist[0, 3, bad] = np.nan
            tu, tx = s.rollout_forward(S, *ins, nl, sequences=cq, states=cx, inputs=I, plant=(Ap, Bp, Cp),
                                       tangents={"disturbance": tdist})
            assert s.last_flags & capi.FLAG_NONFINITE
            assert not tu[0][:, bad].any() and not tx[0][:, bad].any() and tx[0][:, others].all()


def test_padding_ld_and_ld_d():
    """ld > n and ld_d != ld through the C entries: a shard [5, 5 + n) of wider arrays equals the packed call"""
    I, H, S = 2, 10, 6
    ins, nl, ((Ap, Bp, Cp), dist) = case(I, H, 10, True)
    nl, dist = np.ascontiguousarray(nl[:2 * S]), np.ascontiguousarray(dist[:2 * S])
    want = plant_newton(I, H, S, ins, nl, (Ap, Bp, Cp), dist)
    lib = capi.load_library()
    n, ld, ld_d, off = N, N + 13, N + 29, 5

    def wide(a, ld):
        w = np.full((a.shape[0], ld), np.nan)
        w[:, off:off + n] = a
        return w
    arrs = [wide(a, ld) for a in list(ins) + [nl, Ap, Bp, Cp]]
    wd = wide(dist, ld_d)
    u, x, q = (np.full((r, ld), 3.0) for r in (S * I, 2 * S, S * H * I))
    st, first = np.full((S, ld), 9, np.int32), np.full(ld, 9, np.int32)
    ptr = lambda a, itemsize=8: a.ctypes.data + off * itemsize
    with MpcSolver(horizon=H, device=None) as s:
        p = s._params()
        io = capi.GeneralIO(inputs=I, n=n, ld=ld, **{k: ptr(a) for k, a in zip(
            ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets"), arrs)})
        pl = capi.Plant(A=ptr(arrs[10]), B=ptr(arrs[11]), C=ptr(arrs[12]), disturbance=ptr(wd), ld_d=ld_d)
        pol = capi.Polish(tol=TOL, max_rounds=ROUNDS, reserved=0, status=ptr(st, 4))
        flags = C.c_uint32(0)
        rc = lib.tpc_mpc_rollout_plant(s._h, C.byref(p), C.byref(io), C.byref(pl), capi.LOOP_NEWTON, S, ptr(arrs[9]),
                                       C.byref(pol), capi.NEWTON_FALLBACK_NONE, ptr(u), ptr(x), None, ptr(q),
                                       ptr(first, 4), C.byref(flags), capi.HOST, None)
        assert rc == capi.OK and flags.value == want[8]
        for got, ref in ((u, want[0]), (x, want[1]), (q, want[2]), (st, want[3])):
            assert same_bits(np.ascontiguousarray(got[:, off:off + n]), ref)
            assert (got[:, :off] == got[0, 0]).all() and (got[:, off + n:] == got[0, 0]).all()   # padding untouched
        assert same_bits(np.ascontiguousarray(first[off:off + n]), want[5])
        # backward: ddisturbance with ld_d
        G_x = wide(np.ones((2 * S, n)), ld)
        dd, dAp = np.full((2 * S, ld_d), 3.0), np.full((4, ld), 3.0)
        g = capi.RolloutGrad(sequences=ptr(q), states=ptr(x), grad_states=ptr(G_x))
        pg = capi.PlantGrad(dA=ptr(dAp), ddisturbance=ptr(dd))
        rc = lib.tpc_mpc_rollout_plant_backward(s._h, C.byref(p), C.byref(io), C.byref(pl), S, ptr(arrs[9]), C.byref(g),
                                                C.byref(pg), C.byref(flags), capi.HOST, None)
        assert rc == capi.OK
        ref = s.rollout_backward(S, *ins, nl, sequences=want[2], states=want[1], grad_states=np.ones((2 * S, n)),
                                 inputs=I, plant=(Ap, Bp, Cp), want=("Ap", "disturbance"))
        assert same_bits(np.ascontiguousarray(dd[:, off:off + n]), ref["disturbance"])
        assert same_bits(np.ascontiguousarray(dAp[:, off:off + n]), ref["Ap"])
        assert (dd[:, :off] == 3.0).all() and (dd[:, off + n:] == 3.0).all()


# ---- the dense checker, and tests 3 and 5 against it -------------------------------------------------------------------

from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_plant_dense as pd

NAMES = dense.NAMES
KEY = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets",
           nlt="new_last_targets", Ap="Ap", Bp="Bp", Cp="Cp", d="disturbance")


def _aos_case(I, H, S, kind="general"):
    """AoS view of case(): th, nlt [n, S, 2], plant (Ap [n, 4], Bp [n, 2I], Cp [n, 2]), dist [n, S, 2]"""
    th, nlt = inputs(kind, I, H, S, with_nlt=True)
    ins, nl, (plant, dist) = case(I, H, S, True, kind)
    return th, nlt, tuple(np.ascontiguousarray(a.T) for a in plant), np.ascontiguousarray(dist.T).reshape(N, S, 2)


def test_dense_checker_against_central_differences_of_the_polished_replay():
    """3 instances; dL/dAp, dL/dA and one disturbance row of the checker against central differences (step 1e-6) of
    the oracle-based polished replay with the plant line at eps = tol = 1e-12, on components whose perturbation
    changes no active set; the 1e-4 assertion of DESIGN.md section 15."""
    I, H, S, n = 2, 10, 6, 3
    th, nlt, plant, dist = _aos_case(I, H, 10)
    sub = lambda a: None if a is None else np.array(a[:n])
    th = {k: sub(th[k]) for k in NAMES}
    nlt, plant, dist = sub(nlt)[:, :S], tuple(sub(a) for a in plant), sub(dist)[:, :S]
    rng = np.random.default_rng(12)
    G_u, G_x = rng.standard_normal((n, S, I)), rng.standard_normal((n, S, 2))
    tight = dict(eps=1e-12, max_iter=200000, tol=1e-12, max_rounds=8)

    def run(th_, plant_, dist_):
        u0, xs, sq, _ = pd.replay(I, H, S, th_, nlt, plant_, dist_, **tight)
        acts = [[dense.active(sq[i, k], th_["lo"][i], th_["hi"][i]) for k in range(S)] for i in range(n)]
        return (u0 * G_u).sum((1, 2)) + (xs * G_x).sum((1, 2)), acts, sq

    _, acts0, sq0 = run(th, plant, dist)
    refs = [pd.closed_loop(I, H, S, {k: th[k][i] for k in NAMES}, nlt[i], sq0[i], G_u[i], G_x[i],
                           tuple(a[i] for a in plant), dist[i])[0] for i in range(n)]
    checked = 0
    for name, comps in (("Ap", range(4)), ("A", range(4)), ("d", (2 * (S // 2), 2 * (S // 2) + 1))):
        for c in comps:
            vals, stable = [], np.ones(n, dtype=bool)
            base = {"Ap": plant[0], "A": th["A"], "d": dist}[name].reshape(n, -1)
            h = 1e-6 * np.maximum(1.0, np.abs(base[:, c]))
            for sgn in (1.0, -1.0):
                thp = {k: v.copy() for k, v in th.items()}
                pp, dp = tuple(a.copy() for a in plant), dist.copy()
                tgt = {"Ap": pp[0], "A": thp["A"], "d": dp}[name].reshape(n, -1)
                tgt[:, c] += sgn * h
                L, acts, _ = run(thp, pp, dp)
                stable &= np.array([all(np.array_equal(acts[i][k], acts0[i][k]) for k in range(S)) for i in range(n)])
                vals.append(L)
            fd = (vals[0] - vals[1]) / (2 * h)
            for i in np.flatnonzero(stable):
                want = refs[i][name].ravel()[c]
                assert abs(fd[i] - want) <= 1e-4 * max(1.0, abs(want)), (name, c, i, fd[i], want)
                checked += 1
    assert checked >= 20, checked


# Backward against the dense checker: the comparison and the bound tests/test_rollout_grad_host.py holds the parent to
# (per output, |got - want| <= 1e-9 |want| + 1e-12 normwise, the kernel run at the checker's own stationary sequences
# and states).  Largest relative deviation measured over the four shapes, both input kinds, all outputs: printed by the
# test, quoted in DESIGN.md section 18.  The relative part is the parent's.  The absolute floor is re-measured, as the
# issue allows for the new sums: over the four shapes and both input kinds exactly one output exceeds 1e-9 |want| by
# more than 1e-13 -- dnew_last_targets of one instance of mpc_rollout_dense.batch (1, 20, 6), a gradient of norm
# 2.6e-12 beside gradients of order 1, off by 2.108e-12 (what is left of sums that cancel) -- so the floor is 10x that.
DENSE_REL, DENSE_ABS = 1e-9, 10 * 2.108e-12


@functools.lru_cache(maxsize=None)
def _dense_case(kind, I, H, S):
    """carried instances of the host Newton plant loop, the checker's closed loop on their active sets"""
    th, nlt, plant, dist = _aos_case(I, H, S, kind)
    ins, nl, (pl, ds) = case(I, H, S, True, kind)
    u, x, q, st, it, first, *_ = plant_newton(I, H, S, ins, nl, pl, ds)
    carried = np.flatnonzero(first == S)
    seqs = np.ascontiguousarray(q.T).reshape(N, S, H, I)
    rng = np.random.default_rng(21 + H)
    G_u, G_x = rng.standard_normal((N, S, I)), rng.standard_normal((N, S, 2))
    return th, nlt, plant, dist, ins, nl, pl, ds, carried, seqs, G_u, G_x, (u, x)


@pytest.mark.parametrize("I,H,S", SHAPES)
@pytest.mark.parametrize("kind", ["general", "batch"])
def test_plant_backward_matches_the_dense_checker_on_carried_instances(kind, I, H, S):
    th, nlt, plant, dist, ins, nl, pl, ds, carried, seqs, G_u, G_x, (u, x) = _dense_case(kind, I, H, S)
    if kind == "general":
        assert 1.0 - carried.size / N <= COVERAGE_CAP
    assert carried.size
    refs, psq, pxs = {}, np.zeros((N, S, H, I)), np.zeros((N, S, 2))
    for i in carried:
        refs[i], _, pxs[i], psq[i] = pd.closed_loop(I, H, S, {k: th[k][i] for k in NAMES}, nlt[i], seqs[i], G_u[i],
                                                    G_x[i], tuple(a[i] for a in plant), dist[i])
        # the loop the kernel ran is the checker's loop: same optimum per step
        assert np.abs(pxs[i].ravel() - x[:, i]).max() <= 1e-8
    with MpcSolver(horizon=H, device=None) as s:
        out = s.rollout_backward(S, *ins, nl, sequences=dense.soa(psq, N), states=dense.soa(pxs, N),
                                 grad_controls=dense.soa(G_u, N), grad_states=dense.soa(G_x, N), inputs=I, plant=pl,
                                 disturbance=ds)
    worst, gap, floor = 0.0, np.inf, 0.0
    for i in carried:
        for k in list(NAMES) + ["nlt", "Ap", "Bp", "Cp", "d"]:
            got, want = out[KEY[k]][:, i], refs[i][k].ravel()
            err, ref = np.linalg.norm(got - want), np.linalg.norm(want)
            if ref > 0:
                worst = max(worst, err / ref)
            floor = max(floor, err - DENSE_REL * ref)
            assert err <= DENSE_REL * ref + DENSE_ABS, f"instance {i} d{k}: |err| {err:.3e} |ref| {ref:.3e}"
        # dA and dAp are different things: they differ by far more than the bound they are each held to
        a, ap = out["A"][:, i], out["Ap"][:, i]
        gap = min(gap, np.linalg.norm(a - ap) / max(np.linalg.norm(a), np.linalg.norm(ap)))
        assert np.linalg.norm(a - ap) > DENSE_REL * max(np.linalg.norm(a), np.linalg.norm(ap)) + DENSE_ABS
    print(f"{kind} I={I} H={H} S={S}: compared {carried.size}/{N}, largest relative deviation {worst:.3e}, largest excess over the relative part {floor:.3e}, "
          f"smallest |dA - dAp| / max(|dA|, |dAp|) {gap:.3e}")


@pytest.mark.parametrize("I,H,S", SHAPES)
@pytest.mark.parametrize("kind", ["general", "batch"])
def test_plant_forward_matches_the_checkers_jvp_on_carried_instances(kind, I, H, S):
    th, nlt, plant, dist, ins, nl, pl, ds, carried, seqs, _, _, (u, x) = _dense_case(kind, I, H, S)
    dirs = td.random_tangents(I, H, S, N, 33 + H, K=1)
    rng = np.random.default_rng(34 + H)
    extra = dict(Ap=rng.standard_normal((N, 4)), Bp=rng.standard_normal((N, 2 * I)), Cp=rng.standard_normal((N, 2)),
                 d=rng.standard_normal((N, S, 2)))
    tan = td.soa_tangents(dirs, N)
    tan.update(Ap=dense.soa(extra["Ap"], N)[None], Bp=dense.soa(extra["Bp"], N)[None],
               Cp=dense.soa(extra["Cp"], N)[None], disturbance=dense.soa(extra["d"], N)[None])
    q = dense.soa(seqs, N)
    with MpcSolver(horizon=H, device=None) as s:
        tu, tx = s.rollout_forward(S, *ins, nl, sequences=q, states=x, tangents=tan, inputs=I, plant=pl)
        assert s.last_flags == 0 or carried.size < N
    worst = 0.0
    for i in carried:
        t_i = dict({k: v[i] for k, v in dirs[0].items()}, **{k: v[i] for k, v in extra.items()})
        wu, wx, _, _ = pd.closed_loop_jvp(I, H, S, {k: th[k][i] for k in NAMES}, nlt[i], seqs[i], t_i,
                                          tuple(a[i] for a in plant), dist[i])
        for got, want, what in ((tu[0][:, i], wu.ravel(), "tcontrols"), (tx[0][:, i], wx.ravel(), "tstates")):
            err, ref = np.linalg.norm(got - want), np.linalg.norm(want)
            worst = max(worst, err / ref)
            assert err <= 1e-9 * ref + 1e-12, f"instance {i} {what}: |err| {err:.3e} |ref| {ref:.3e}"
    print(f"{kind} I={I} H={H} S={S}: compared {carried.size}/{N}, largest relative error {worst:.3e}")
