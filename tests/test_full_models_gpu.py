"""`-m gpu` tests of every general-form kernel on FULL 2x2 models (tests/model/full_models.py: every entry of A and B
live; complex, stable, unstable, negative-determinant, nearly-shipped and singular A).  The rest of the suite feeds them
A = [1, Tv; 0, 1] almost everywhere, where a dropped a10 term, a00 and a11 exchanged, a lost b00, a wrong (1,0) entry of
a squared matrix power or a transposed product with its mixed terms exchanged cannot be seen.

Each family is held to ITS existing criterion, unchanged: bits and iteration counts for LANE (both layouts) and the
generic kernel, |du| <= 1e-9 with equal counts for WAVE, LANE_FMA and GROUP; against the oracle on a batch of 131 (a
last partial wavefront) and against real dlib's recorded answers (general_full_*.npz, rollout_full_*.npz:
tests/golden/make_golden_full.py).  The derivative, polish and closed-loop entries make their existing statement --
DEVICE memory equals the host-only handle byte for byte -- and tests/test_full_models_host.py holds the host side to
the dense references on the same family."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, load_golden
from tests.model import decision_cases as dc
from tests.model import full_models as fm
from tests.model import mpc_rollout_tangent_dense as td
from tests.test_decision_edges_gpu import _check, _expected, _family as pinned, _solve
from tests.test_rollout_plant_gpu import _composed as composed_plant
from tests.test_rollout_polish_gpu import _composed as composed_polished, _fused as fused_polished
from trajectory_controller_amd import MpcSolver, capi, mpc_general, mpc_rollout

pytestmark = pytest.mark.gpu

ATOL = 1e-9
GROUP = 4
ALWAYS, NEVER = 1 << 40, 0
NAMES = fm.NAMES
N = 131
TOL, ROUNDS = 1e-9, 8
GROUPS = [(10, 2), (10, 4), (20, 2), (20, 4), (20, 8), (30, 2), (30, 4), (30, 8), (40, 2), (40, 4), (40, 8)]
WAVE_SHAPES = [(2, 4), (1, 10), (2, 10), (1, 30), (2, 30), (2, 40)]


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _g(I, H, n=N):
    return fm.full_models(I, H, n)


def _want(orc, I, H, tag="cold", g=None, cin=None, **kw):
    return _expected(orc, f"full_models:{tag}", I, H, _g(I, H) if g is None else g, cin, **kw)


# ---- solver families, cold start -------------------------------------------------------------------------------------

@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H", [4, 5, 10, 20, 30, 40])
def test_lane_fp64_bits(torch_cuda, oracle, I, H):
    g, fx = _g(I, H), load_golden(f"general_full_I{I}_H{H}.npz")
    for below in ([ALWAYS, NEVER] if H >= 10 else [NEVER]):
        with pinned(H, ("lanex", below)) as s:
            _check("lane", _solve(s, g, I, H), _want(oracle, I, H), what=f"below {below}")
            u0 = _solve(s, fx, I, H)[0]
        assert bits_equal(u0, fx["u0"]), below


@pytest.mark.parametrize("I,H", [(2, 5), (2, 20)])
def test_lane_fp32_bits(torch_cuda, oracle32, I, H):
    g = {k: v.astype(np.float32) for k, v in _g(I, H).items()}
    with pinned(H, "lane", dtype="f32") as s:
        _check("lane", _solve(s, g, I, H, np.float32), _want(oracle32, I, H, "f32", g), np.float32)


@pytest.mark.parametrize("I,H,dtype", [(1, 1, "f64"), (2, 7, "f64"), (1, 33, "f64"), (2, 64, "f64"), (2, 7, "f32")])
def test_generic_bits(torch_cuda, oracle, oracle32, I, H, dtype):
    npdt, orc = (np.float64, oracle) if dtype == "f64" else (np.float32, oracle32)
    g = {k: v.astype(npdt) for k, v in _g(I, H).items()}
    with pinned(H, "generic", dtype=dtype) as s:
        _check("generic", _solve(s, g, I, H, npdt), _want(orc, I, H, dtype, g), npdt)


@pytest.mark.parametrize("I,H", WAVE_SHAPES)
def test_wave_fp64(torch_cuda, oracle, I, H):
    """four, two and one instance per wavefront; TPC_MPC_OPT_WAVE_GROUP 0 and 1 give the same bits"""
    g, fx = _g(I, H), load_golden(f"general_full_I{I}_H{H}.npz")
    got = []
    for grp in (0, 1):
        with pinned(H, ("wave", grp)) as s:
            got.append(_solve(s, g, I, H))
            _check("wave", got[-1], _want(oracle, I, H), what=f"wave_group {grp}")
            u0 = _solve(s, fx, I, H)[0]
        assert np.abs(u0 - fx["u0"]).max() <= ATOL
    assert bits_equal(got[0][0], got[1][0]) and np.array_equal(got[0][2], got[1][2])


def test_wave_fp32(torch_cuda, oracle32):
    """the tolerance of tests/test_parity_gpu.py::test_wave_fp32_vs_float_typed_oracle at H = 10"""
    I, H, n = 2, 10, 1024
    g = {k: v.astype(np.float32) for k, v in fm.full_models(I, H, n).items()}
    ou0, _, oit = oracle32.solve_general(I, H, *[g[k] for k in NAMES], nthreads=8)
    with pinned(H, "wave", dtype="f32") as s:
        u0, _, it, _ = _solve(s, g, I, H, np.float32)
    err = np.abs(u0 - ou0).max(axis=1)
    same = float(np.mean(it == oit))
    print(f"WAVE fp32 full models: equal counts {same:.4f}; |du| median {np.median(err):.2e} p99 {np.quantile(err, 0.99):.2e}")
    assert same >= 0.8 and np.median(err) <= 2e-5 and np.quantile(err, 0.99) <= 5e-3


@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H", [4, 5, 10, 20])
def test_lane_fma(torch_cuda, oracle, I, H):
    g, fx = _g(I, H), load_golden(f"general_full_I{I}_H{H}.npz")
    with pinned(H, "lane_fma") as s:
        _check("lane_fma", _solve(s, g, I, H), _want(oracle, I, H))
        u0 = _solve(s, fx, I, H)[0]
    assert np.abs(u0 - fx["u0"]).max() <= ATOL


@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H,G", GROUPS)
def test_group_general(torch_cuda, oracle, I, H, G):
    """every group size, the padded chunks of (10, 4), (30, 4), (30, 8) included: A^L, A^2L, A^4L and their
    transposes with a live (1,0) entry"""
    g, fx = _g(I, H), load_golden(f"general_full_I{I}_H{H}.npz")
    with pinned(H, ("group", G)) as s:
        _check("group", _solve(s, g, I, H, expect_algo=GROUP), _want(oracle, I, H), what=f"G {G}")
        u0 = _solve(s, fx, I, H, expect_algo=GROUP)[0]
    assert np.abs(u0 - fx["u0"]).max() <= ATOL


def test_auto_capped_instances_carry_dlibs_bits(torch_cuda, oracle):
    """max_iter lowered until class 4 (and others) end on the cap: AUTO re-solves those with the bit-exact kernels"""
    I, H, cap = 2, 40, 1000
    g = _g(I, H)
    wu0, _, wit, _ = _want(oracle, I, H, "capped", max_iter=cap)
    capped = wit >= cap
    assert capped[fm.model_class(N) == 4].any() and not capped.all()
    with pinned(H, "auto", max_iter=cap) as s:
        u0, _, it, _ = _solve(s, g, I, H)
        flags = s.last_flags
    assert np.array_equal(it, wit)
    assert bits_equal(u0[capped], wu0[capped])
    assert np.abs(u0 - wu0).max() <= ATOL
    assert bool(flags & capi.FLAG_MAX_ITER) == bool(capped.any())
    # the other half of the iff: where the oracle caps nowhere the flag stays clear
    wit = _want(oracle, I, 20)[2]
    assert not (wit >= 10000).any()
    with pinned(20, "auto") as s:
        _check("auto", _solve(s, _g(I, 20), I, 20), _want(oracle, I, 20))
        assert s.last_flags & capi.FLAG_MAX_ITER == 0


# ---- state in and out --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", [("lanex", ALWAYS), ("lanex", NEVER), "wave", ("group", 4), "generic"],
                         ids=["lanex", "lane", "wave", "group", "generic"])
@pytest.mark.parametrize("I,H", [(2, 10), (1, 20)])
def test_state_in_and_out(torch_cuda, oracle, family, I, H):
    """warm starts partly outside the box and a random v: outputs, the whole sequence, dlib's v and the counts"""
    Hk = H if family != "generic" else H + 1       # the generic kernel runs the horizons without a specialised one
    g = _g(I, Hk)
    cin, vin = fm.warm_start(I, Hk, N)
    want = oracle.solve_general(I, Hk, *[g[k] for k in NAMES], controls_in=cin, v_in=vin, want_v=True, nthreads=8)
    controls, vstate = fm.soa(cin), fm.soa(vin)
    with pinned(Hk, family) as s:
        s.set_profiling(True)
        u0, it = s.solve_batch_general(*[fm.soa(g[k]) for k in NAMES], controls=controls, v_state=vstate, inputs=I,
                                       want_iters=True)
        if family == ("group", 4):
            assert s.last_kernel_times()[2] == GROUP
    got = (u0.T, dc.aos(controls, Hk, I), it, dc.aos(vstate, Hk, I))
    _check(family, got, want, what="warm")


# ---- the hostile variant -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["wave", "lane_fma", ("group", 4), "generic"], ids=["wave", "lane_fma", "group", "generic"])
def test_hostile(torch_cuda, oracle, family):
    """The companion of test_lanex_general_hostile.  For GROUP this is the REFUSED path, not the group arithmetic: the
    stop-test screen refuses a batch with pinned or one-sided boxes and the one-lane exact build solves it on GROUP's
    records (tests/test_groupg_gpu.py::test_groupg_hostile_batch_takes_the_exact_kernels), here with full models;
    GROUP's own scans are held by test_group_general, test_state_in_and_out[group] and test_rollout_fixtures."""
    I, H = 2, (20 if family != "generic" else 21)
    g = fm.hostile({k: v.copy() for k, v in _g(I, H).items()}, I)
    want = _want(oracle, I, H, "hostile", g)
    with pinned(H, family) as s:
        _check(family, _solve(s, g, I, H), want, what="hostile")


# ---- rollout -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("H", [4, 5, 10, 20, 30, 40])
def test_rollout_fixtures(torch_cuda, I, H):
    """real dlib's 12 controllers x 5 warm-started steps on full models: LANE bits (controls and the states of
    x <- A x + B u + C with a live a10), WAVE and GROUP within dlib's own 1e-7 (tests/test_groupg_gpu.py)"""
    g = load_golden(f"rollout_full_I{I}_H{H}.npz")
    steps, n = int(g["steps"]), g["A"].shape[0]
    args = [fm.soa(g[k]) for k in NAMES]
    for algo in ("lane", "wave") + (("group",) if H >= 10 else ()):
        with MpcSolver(horizon=H, device=0, algo=algo) as s:
            s.set_profiling(True)
            c, st, _ = s.rollout(steps, *args, new_last_targets=fm.soa(g["new_last_targets"]), inputs=I)
            if algo == "group":
                assert s.last_kernel_times()[2] == GROUP
        c, st = c.T.reshape(n, steps, I), st.T.reshape(n, steps, 2)
        if algo == "lane":
            assert bits_equal(c, g["controls"]) and bits_equal(st, g["states"])
        else:
            assert np.abs(c - g["controls"]).max() <= 1e-7 and np.abs(st - g["states"]).max() <= 1e-7, algo


def test_rollout_generic(torch_cuda, oracle):
    I, H, S, n = 2, 7, 4, 36
    g = _g(I, H, n)
    nlt = fm.new_last_targets(g, S)
    with MpcSolver(horizon=H, device=0) as s:
        c, st, it = s.rollout(S, *[fm.soa(g[k]) for k in NAMES], new_last_targets=fm.soa(nlt), inputs=I, want_iters=True)
    for k in range(n):
        wc, ws, wit = oracle.rollout(I, H, S, *[g[key][k] for key in NAMES], nlt[k])
        assert bits_equal(c[:, k].reshape(S, I), wc) and bits_equal(st[:, k].reshape(S, 2), ws), k
        assert np.array_equal(it[:, k], wit), k


# ---- derivative, polish and closed-loop entries: DEVICE memory against the host-only handle, byte for byte -----------

SHAPES = [(2, 5), (2, 20), (1, 33)]
S = 4


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def down(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same(a, b):
    a, b = np.ascontiguousarray(down(a)), np.ascontiguousarray(down(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _loop_case(I, H):
    g = _g(I, H)
    ins, nl = [fm.soa(g[k]) for k in NAMES], fm.soa(fm.new_last_targets(g, S, seed=H))
    *plant, dist = fm.full_plant(g, 0.05, steps=S)
    return g, ins, nl, tuple(fm.soa(a) for a in plant), fm.soa(dist)


@pytest.mark.parametrize("I,H", SHAPES)
def test_backward_forward_polish_equal_the_host_path(torch_cuda, oracle, I, H):
    g = _g(I, H)
    ins = [fm.soa(g[k]) for k in NAMES]
    _, ctl, _ = oracle.solve_general(I, H, *[g[k] for k in NAMES], nthreads=8)
    loose = fm.soa(ctl)
    rng = np.random.default_rng(H)
    G = rng.standard_normal((H * I, N))
    tan = td.soa_tangents(td.random_tangents(I, H, 1, N, 8, with_nlt=False, K=3), N)
    with MpcSolver(horizon=H, device=None) as hs:
        wu = loose.copy()
        _, wst, wri, wro = hs.polish_batch_general(*ins, wu, tol=TOL, max_rounds=ROUNDS, inputs=I)
        wg = hs.solve_batch_general_backward(*ins, wu, G, inputs=I)
        wt = hs.solve_batch_general_forward(*ins, wu, tan, inputs=I)
    assert (wst >= 0).mean() >= 0.75
    with MpcSolver(horizon=H, device=0) as s:
        dins, u = [up(a) for a in ins], up(loose)
        _, st, ri, ro = s.polish_batch_general(*dins, u, tol=TOL, max_rounds=ROUNDS, inputs=I)
        assert same(u, wu) and same(st, wst) and same(ri, wri) and same(ro, wro)
        dg = s.solve_batch_general_backward(*dins, up(wu), up(G), inputs=I)
        for k in wg:
            assert same(dg[k], wg[k]), k
        assert same(s.solve_batch_general_forward(*dins, up(wu), {k: up(v) for k, v in tan.items()}, inputs=I), wt)


@pytest.mark.parametrize("I,H", SHAPES)
def test_recorded_rollout_and_its_derivatives(torch_cuda, oracle, I, H):
    """rollout_record (the bit-exact kernels: the oracle's closed loop), then rollout_backward and rollout_forward at
    the recorded loop, DEVICE memory against the host-only handle"""
    g, ins, nl, _, _ = _loop_case(I, H)
    nlt = fm.new_last_targets(g, S, seed=H)
    rng = np.random.default_rng(2)
    G_u, G_x = rng.standard_normal((S * I, N)), rng.standard_normal((2 * S, N))
    tan = td.soa_tangents(td.random_tangents(I, H, S, N, 8, K=3), N)
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        u, x, q, it = s.rollout_record(S, *ins, nl, inputs=I, want_iters=True)
        for k in range(0, N, 5):
            wc, ws, wit = oracle.rollout(I, H, S, *[g[key][k] for key in NAMES], nlt[k])
            assert bits_equal(u[:, k].reshape(S, I), wc) and bits_equal(x[:, k].reshape(S, 2), ws), k
        dins, dnl = [up(a) for a in ins], up(nl)
        dg = s.rollout_backward(S, *dins, dnl, sequences=up(q), states=up(x), grad_controls=up(G_u),
                                grad_states=up(G_x), inputs=I)
        dt = s.rollout_forward(S, *dins, dnl, sequences=up(q), states=up(x), tangents={k: up(v) for k, v in tan.items()},
                               inputs=I)
    with MpcSolver(horizon=H, device=None) as hs:
        wg = hs.rollout_backward(S, *ins, nl, sequences=q, states=x, grad_controls=G_u, grad_states=G_x, inputs=I)
        wt = hs.rollout_forward(S, *ins, nl, sequences=q, states=x, tangents=tan, inputs=I)
    for k in wg:
        assert same(dg[k], wg[k]), k
    assert same(dt[0], wt[0]) and same(dt[1], wt[1])


@pytest.mark.parametrize("I,H", SHAPES)
def test_rollout_polished_equals_its_composed_loop(torch_cuda, I, H):
    g, ins, nl, _, _ = _loop_case(I, H)
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        want = composed_polished(s, I, H, S, ins, nl, True, TOL, ROUNDS)
        got, _ = fused_polished(s, I, H, S, ins, nl, True, TOL, ROUNDS)
    assert (want[3] >= 0).mean() >= 0.75
    for a, b in zip(got, want):
        assert same(a, b)


@pytest.mark.parametrize("with_plant", [False, True], ids=["newton", "plant"])
@pytest.mark.parametrize("I,H", SHAPES)
def test_newton_loop_and_plant_loops(torch_cuda, I, H, with_plant):
    """FALLBACK_NONE: DEVICE bytes against the host-only handle, with its backward and forward; FALLBACK_SOLVE:
    rollout_polished on the gathered instances; with the additive plant also LOOP_RECORD and LOOP_POLISHED against
    the loop composed from the public entries."""
    g, ins, nl, plant, dist = _loop_case(I, H)
    if not with_plant:
        plant = dist = None
    kw = dict(inputs=I, tol=TOL, max_rounds=ROUNDS, want_iters=True)
    rng = np.random.default_rng(3)
    G_u, G_x = rng.standard_normal((S * I, N)), rng.standard_normal((2 * S, N))
    tan = td.soa_tangents(td.random_tangents(I, H, S, N, 8, K=3), N)
    if with_plant:
        tan.update(Ap=rng.standard_normal((3, 4, N)), Bp=rng.standard_normal((3, 2 * I, N)),
                   Cp=rng.standard_normal((3, 2, N)), disturbance=rng.standard_normal((3, 2 * S, N)))
    with MpcSolver(horizon=H, device=None) as hs:
        want = hs.rollout_newton(S, *ins, nl, fallback="none", plant=plant, disturbance=dist, **kw)
        wflags = hs.last_flags
        u, x, q = want[:3]
        wg = hs.rollout_backward(S, *ins, nl, sequences=q, states=x, grad_controls=G_u, grad_states=G_x, inputs=I,
                                 plant=plant, disturbance=dist)
        wt = hs.rollout_forward(S, *ins, nl, sequences=q, states=x, tangents=tan, inputs=I, plant=plant)
    assert (want[5] == S).mean() >= 0.75
    dpl = None if plant is None else tuple(up(a) for a in plant)
    dds = None if dist is None else up(dist)
    with MpcSolver(horizon=H, device=0, algo="lane") as s:
        dins, dnl = [up(a) for a in ins], up(nl)
        got = s.rollout_newton(S, *dins, dnl, fallback="none", plant=dpl, disturbance=dds, **kw)
        assert s.last_flags == wflags
        for a, b in zip(got, want):
            assert same(a, b)
        dg = s.rollout_backward(S, *dins, dnl, sequences=up(q), states=up(x), grad_controls=up(G_u),
                                grad_states=up(G_x), inputs=I, plant=dpl, disturbance=dds)
        for k in wg:
            assert same(dg[k], wg[k]), k
        dt = s.rollout_forward(S, *dins, dnl, sequences=up(q), states=up(x), tangents={k: up(v) for k, v in tan.items()},
                               inputs=I, plant=dpl)
        assert same(dt[0], wt[0]) and same(dt[1], wt[1])
        # FALLBACK_SOLVE: the stopped instances are the polished loop's, the carried ones keep their bytes
        full = s.rollout_newton(S, *ins, nl, fallback="solve", plant=plant, disturbance=dist, **kw)
        pol = s.rollout_polished(S, *ins, nl, plant=plant, disturbance=dist, **kw)
        fb = want[5] < S
        for i in range(5):
            assert same(full[i][:, fb], pol[i][:, fb]) and same(full[i][:, ~fb], want[i][:, ~fb]), i
        if with_plant:
            for polished in (False, True):
                ref = composed_plant(s, I, H, S, ins, nl, plant, dist, polished)
                c, v = np.zeros((H * I, N)), np.zeros((H * I, N))
                if polished:
                    lu, lx, lq, lst, lit = s.rollout_polished(S, *ins, nl, controls=c, v_state=v, plant=plant,
                                                              disturbance=dist, **kw)
                else:
                    lu, lx, lq, lit = s.rollout_record(S, *ins, nl, controls=c, v_state=v, inputs=I, want_iters=True,
                                                       plant=plant, disturbance=dist)
                    lst = None
                for a, b in zip((lu, lx, lq, lit, lst, c, v), ref):
                    assert (a is None and b is None) or same(a, b), polished


def test_autograd_equals_the_raw_entries(torch_cuda):
    """mpc_general and mpc_rollout on a full model: backward and jvp are the raw entries' bytes"""
    from tests.test_rollout_tangent_gpu import _dual_run
    I, H = 2, 10
    g, ins, nl, _, _ = _loop_case(I, H)
    rng = np.random.default_rng(4)
    names = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "new_last_targets")
    leaves = [up(a) for a in ins] + [up(nl)]
    tans = [up(rng.standard_normal(tuple(a.shape))) for a in leaves]
    with MpcSolver(horizon=H, device=0) as s:
        # the single solve
        fn = lambda *a: mpc_general(s, *a)
        (u,), (tu,) = _dual_run(fn, leaves[:9], tans[:9])
        direct = s.solve_batch_general_forward(*leaves[:9], u, dict(zip(names[:9], tans[:9])), inputs=I)
        assert same(tu, direct[0]) and down(tu).any()
        req = [a.clone().requires_grad_(True) for a in leaves[:9]]
        G = up(rng.standard_normal(tuple(u.shape)))
        grads = torch.autograd.grad((fn(*req) * G).sum(), req)
        raw = s.solve_batch_general_backward(*leaves[:9], u, G, inputs=I)
        for t, k in zip(grads, names):
            assert same(t, raw[k]), k
        # the closed loop
        fn = lambda *a: mpc_rollout(s, S, *a[:9], new_last_targets=a[9])
        (cu, cx), (tcu, tcx) = _dual_run(fn, leaves, tans)
        ru, rx, rq, _ = s.rollout_record(S, *leaves[:9], leaves[9], inputs=I)
        assert same(cu, ru) and same(cx, rx)
        du, dx = s.rollout_forward(S, *leaves[:9], leaves[9], sequences=rq, states=rx, inputs=I,
                                   tangents=dict(zip(names, tans)))
        assert same(tcu, du[0]) and same(tcx, dx[0])
        req = [a.clone().requires_grad_(True) for a in leaves]
        G_u, G_x = up(rng.standard_normal(tuple(cu.shape))), up(rng.standard_normal(tuple(cx.shape)))
        qu, qx = fn(*req)
        grads = torch.autograd.grad((qu * G_u).sum() + (qx * G_x).sum(), req)
        raw = s.rollout_backward(S, *leaves[:9], leaves[9], sequences=rq, states=rx, grad_controls=G_u, grad_states=G_x,
                                 inputs=I)
        for t, k in zip(grads, names):
            assert same(t, raw[k]), k
