"""CPU tests on FULL 2x2 models (tests/model/full_models.py: every entry of A and B live, six classes of A).

Almost every other model the suite feeds the general form is synth.general_inputs' A = [1, Tv; 0, 1]: a10 == 0,
a00 == a11 == 1 and, with two inputs, b00 == 0, so a dropped a10 term, a00 and a11 exchanged or a lost b00 pass it.
Here:
  1. the family keeps what it promises (so that no test on it, here or on the GPU, passes vacuously);
  2. the CPU model of the LANE_FMA arithmetic against the oracle (which tests/test_oracle_golden.py pins to real dlib
     on this family): equal iteration counts, |du| <= UB_ATOL;
  3. the host-only handle's derivative, polish and closed-loop entries against the dense references.

Tolerance of part 3, from the references alone: normwise |got - ref| <= max(1e-8, 16 * 2^-53 * cond(H_FF)) * |ref|
(the closed loops' GRADIENTS add the absolute floor of tests/test_rollout_grad_host.py, 1e-12: a gradient that is zero
in exact arithmetic -- of a bound no step touches, of a new_last_targets row no horizon reaches -- is rounding in both;
controls, states and tangents are held to the relative bound alone).
1e-8 is what tests/test_grad_host.py holds the single solve to; the second term is the dense reference's own loss (a
Gaussian solve with H_FF loses cond(H_FF) units of rounding; 16 of them are allowed) and takes over above cond =
5.6e6, which only H >= 40 reaches here.  For a closed loop the condition number is the largest over the loop's steps.
The worst error and its condition number are printed per shape and quoted in NOTEBOOK.md.

The Newton-first and plant loops are held to mpc_rollout_plant_dense.closed_loop on the loop's own active sets -- the
exact stationary point of every step -- not to the oracle-and-polish replay of mpc_rollout_polish_ref: that replay
polishes with the host polish entry itself (the code under test) and agrees with the loop only to the sum of two
deviations from the same stationary point, so it is the weaker and the less independent statement.
"""
import functools

import numpy as np
import pytest

from tests.model import full_models as fm
from tests.model import mpc_grad_dense as dense
from tests.model import mpc_polish_dense as pdense
from tests.model import mpc_rollout_dense as rd
from tests.model import mpc_rollout_plant_dense as plant_dense
from tests.model import mpc_rollout_tangent_dense as td
from tests.test_rollout_tangent_host import BOUND as IDENTITY_BOUND, mismatch
from tests.test_ub_model import UB_ATOL
from trajectory_controller_amd import MpcSolver, capi

NAMES = fm.NAMES
KEY = dict(A="A", B="B", C="C", Q="Q", R="R", lo="lower", hi="upper", x0="x0", targets="targets",
           nlt="new_last_targets", Ap="Ap", Bp="Bp", Cp="Cp", d="disturbance")
UB_SHAPES = [(1, 4), (2, 5), (2, 10), (1, 20), (2, 20)]
SHAPES = [(1, 4), (2, 5), (2, 10), (2, 20), (2, 40), (1, 64)]
N, S = 24, 4
TIGHT = dict(eps=1e-12, max_iter=200000)
TOL, ROUNDS = 1e-9, 8
PLANT_SCALE = 0.05


def rel_bound(cond):
    return max(1e-8, 16.0 * 2.0 ** -53 * cond)


@pytest.fixture(scope="module")
def model():
    from tests.model.bindings import UbModel
    return UbModel()


@functools.lru_cache(maxsize=None)
def _family(I, H, n):
    return fm.full_models(I, H, n)


@functools.lru_cache(maxsize=None)
def _oracle_solution(I, H, n):
    from oracle.bindings import Oracle
    g = _family(I, H, n)
    return Oracle().solve_general(I, H, *[g[k] for k in NAMES], nthreads=8)


# ---- 1. the family ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("I,H", [(1, 4), (2, 20), (2, 40)])
def test_family_keeps_what_it_promises(I, H):
    n = 600
    g = _family(I, H, n)
    gi = fm.general_inputs(H, n, I=I, first=610000)
    for k in NAMES[2:]:
        assert np.array_equal(g[k], gi[k]), k              # Q, R, bounds, x0, C, targets are general_inputs'
    A, cls = g["A"], fm.model_class(n)
    assert set(cls) == set(range(fm.CLASSES))
    for c in range(5):
        # class 4's e is drawn from [-0.02, 0.02] and may fall below: its other three entries are held, and e != 0
        ent = np.abs(A[cls == c]) if c < 4 else np.abs(A[cls == c][:, [0, 1, 3]])
        live = (ent >= fm.LIVE).all(axis=1)
        print(f"I={I} H={H} class {c}: every |a_ij| >= 0.01 in {live.mean():.3f} of the instances")
        assert live.mean() >= 0.9, (c, live.mean())
    e = np.abs(A[cls == 4][:, 2])
    print(f"I={I} H={H} class 4: |e| {e.min():.2e} .. {e.max():.2e}, >= 0.01 in {np.mean(e >= 0.01):.3f}")
    assert e.min() > 0.0 and np.mean(e >= 0.005) >= 0.5
    sing = A[cls == 5]
    det = sing[:, 0] * sing[:, 3] - sing[:, 1] * sing[:, 2]
    assert np.all(np.abs(det) <= 1e-15 * np.abs(sing).max(axis=1) ** 2)
    assert np.all(np.abs(sing) > 0.0)
    radius = fm.spectral_radius(A)
    print(f"I={I} H={H}: spectral radius {radius.min():.3f} .. {radius.max():.4f}")
    assert radius.max() <= fm.RADIUS_CAP
    assert (radius[cls == 2] >= 1.0).all() and (radius[cls == 5] <= 0.9 + 1e-12).all()
    assert np.all(A[cls == 3, 0] * A[cls == 3, 3] - A[cls == 3, 1] * A[cls == 3, 2] < 0.0)
    assert np.all(g["B"] != 0.0) and np.abs(g["B"] - gi["B"]).min() >= 0.02 - 1e-15
    assert np.abs(g["B"] - gi["B"]).max() <= 0.2
    # what the synthetic model never has
    assert np.all(gi["A"][:, 2] == 0.0) and np.all(A[:, 2] != 0.0)
    unequal = np.isin(cls, (1, 2, 3, 5))                        # (a rotation and class 4 have a00 == a11 by form)
    assert np.all(A[unequal, 0] != A[unequal, 3]) and np.mean(np.abs(A[unequal, 0] - A[unequal, 3]) > 0.01) >= 0.9


@pytest.mark.parametrize("I,H,n", [(I, H, 600) for I, H in UB_SHAPES] + [(2, 30, 120), (2, 40, 120), (1, 40, 120)])
def test_oracle_rarely_ends_on_the_iteration_cap(I, H, n):
    _, _, it = _oracle_solution(I, H, n)
    capped = it >= 10000
    print(f"I={I} H={H}: {int(capped.sum())} of {n} on the cap, classes {sorted(set(fm.model_class(n)[capped]))}, "
          f"median iterations {int(np.median(it))}")
    assert capped.mean() <= 0.10


def test_plant_is_additive_and_live():
    g = _family(2, 10, N)
    Ap, Bp, Cp, d = fm.full_plant(g, PLANT_SCALE, steps=S)
    assert Ap.shape == g["A"].shape and Bp.shape == g["B"].shape and Cp.shape == g["C"].shape and d.shape == (N, S, 2)
    assert np.all(Ap != g["A"]) and np.all(Bp != g["B"]) and np.all(Ap[:, 2] != 0.0)
    # additive: a zero entry of the model would still be moved (the multiplicative plant of the other tests keeps it)
    z = {k: np.zeros_like(g[k]) for k in ("A", "B", "C")}
    assert all(np.all(a != 0.0) for a in fm.full_plant(z, PLANT_SCALE))


def test_hostile_and_warm_start_builders():
    I, H, n = 2, 20, 131
    g = fm.hostile({k: v.copy() for k, v in _family(I, H, n).items()}, I)
    assert np.all(g["hi"][0::11] == g["lo"][0::11]) and np.all(g["B"][2::11, 0::I] == 0.0) and np.all(g["Q"][3::11] == 0.0)
    assert np.all(g["A"] != 0.0)
    cin, vin = fm.warm_start(I, H, n)
    assert cin.shape == vin.shape == (n, H, I)
    assert (np.abs(cin) > 0.384).any() and (np.abs(cin) < 0.3).any()


# ---- 2. the LANE_FMA arithmetic --------------------------------------------------------------------------------------

@pytest.mark.parametrize("I,H", UB_SHAPES)
@pytest.mark.parametrize("fast", [True, False])
def test_ub_model_vs_oracle(model, I, H, fast):
    n = 600
    g = _family(I, H, n)
    ou0, _, oit = _oracle_solution(I, H, n)
    u0, it, _ = model.solve_general(I, H, *[g[k] for k in NAMES], nthreads=8, fast_stop=fast)
    print(f"I={I} H={H} fast_stop={fast}: equal counts {int((it == oit).sum())}/{n}, max |du| {np.abs(u0 - ou0).max():.3e}")
    assert np.array_equal(it, oit)
    assert np.abs(u0 - ou0).max() <= UB_ATOL
    assert np.array_equal((ou0 == g["lo"]) | (ou0 == g["hi"]), (u0 == g["lo"]) | (u0 == g["hi"]))


@pytest.mark.parametrize("I,H", [(1, 10), (2, 20)])
def test_ub_model_hostile(model, oracle, I, H):
    g = fm.hostile({k: v.copy() for k, v in _family(I, H, 440).items()}, I)
    ou0, _, oit = oracle.solve_general(I, H, *[g[k] for k in NAMES], nthreads=8)
    u0, it, flags = model.solve_general(I, H, *[g[k] for k in NAMES], nthreads=8, fast_stop=False)
    assert flags == 0
    assert np.array_equal(it, oit)
    assert np.abs(u0 - ou0).max() <= UB_ATOL


# ---- 3. the host-only handle against the dense references -----------------------------------------------------------

def _ins(th, n=N):
    return [dense.soa(th[k], n) for k in NAMES]


LOOP_FLOOR = 1e-12     # the closed-loop comparisons' absolute floor, that of tests/test_rollout_grad_host.py


def _held(got, want, cond, what, floor=0.0):
    """normwise error relative to the bound; asserts"""
    err, ref = np.linalg.norm(got - want), np.linalg.norm(want)
    assert err <= rel_bound(cond) * ref + floor, f"{what}: |err| {err:.3e} |ref| {ref:.3e} cond(H_FF) {cond:.3e}"
    return err / ref if ref > floor / rel_bound(cond) else 0.0


@functools.lru_cache(maxsize=None)
def _single(I, H):
    """the family, the exact stationary point on the oracle's active set, and keep (mpc_grad_dense.solved)"""
    th = _family(I, H, N)
    _, ustar, keep = dense.solved(I, H, th)
    assert keep.sum() >= 0.75 * N, keep
    return th, ustar, keep


@pytest.mark.parametrize("I,H", SHAPES)
def test_host_backward_and_forward_match_the_dense_reference(I, H):
    th, ustar, keep = _single(I, H)
    g = np.random.default_rng(3).standard_normal((N, H, I))
    dirs = td.random_tangents(I, H, 1, N, 41 + H, with_nlt=False, K=2)
    tan = td.soa_tangents(dirs, N)
    with MpcSolver(horizon=H, device=None) as s:
        out = s.solve_batch_general_backward(*_ins(th), dense.soa(ustar, N), dense.soa(g, N), inputs=I)
        assert s.last_flags == 0
        tu = s.solve_batch_general_forward(*_ins(th), dense.soa(ustar, N), tan, inputs=I)
        assert s.last_flags == 0
    worst, worst_cond, n_act = 0.0, 1.0, 0
    for i in np.flatnonzero(keep):
        t0 = {k: th[k][i] for k in NAMES}
        ref, _, cond, act = dense.instance(I, H, t0, ustar[i], g[i])
        n_act += int(act.any())
        for k in NAMES:
            r = _held(out[KEY[k]][:, i], ref[k].ravel(), cond, f"instance {i} (class {i % 6}) d{k}")
            if r > worst:
                worst, worst_cond = r, cond
        assert out["kkt_residual"][i] < 1e-9
        for d in range(2):
            want, _ = td.instance_jvp(I, H, t0, ustar[i], {k: v[i] for k, v in dirs[d].items()})
            r = _held(tu[d][:, i], want.ravel(), cond, f"instance {i} (class {i % 6}) tangent {d}")
            if r > worst:
                worst, worst_cond = r, cond
    ident = max(float(mismatch([dense.soa(g, N) * tu[d]], [out[k] * tan[k][d] for k in tan]).max()) for d in range(2))
    print(f"I={I} H={H}: kept {int(keep.sum())}/{N}, with active components {n_act}, worst relative error {worst:.3e} at "
          f"cond(H_FF) {worst_cond:.3e}, transpose identity {ident:.3e} (bound {IDENTITY_BOUND:.3e})")
    assert n_act > 0
    assert ident <= IDENTITY_BOUND


@pytest.mark.parametrize("I,H", SHAPES)
def test_host_polish_from_zero_matches_the_dense_checker(I, H):
    th = _family(I, H, N)
    zero = np.zeros((N, H, I))
    u = dense.soa(zero, N).copy()
    with MpcSolver(horizon=H, device=None) as s:
        _, st, ri, ro = s.polish_batch_general(*_ins(th), u, tol=TOL, max_rounds=ROUNDS, inputs=I)
    u = u.T.reshape(N, H, I)
    du, ds, _, _ = pdense.polish_batch(I, H, th, zero, TOL, ROUNDS)
    both = (st >= 0) & (ds >= 0)
    worst, worst_cond = 0.0, 1.0
    for i in np.flatnonzero(both):
        _, _, cond, _ = dense.instance(I, H, {k: th[k][i] for k in NAMES}, du[i], np.zeros((H, I)))
        r = _held(u[i].ravel(), du[i].ravel(), cond, f"instance {i} (class {i % 6})")
        if r > worst:
            worst, worst_cond = r, cond
    print(f"I={I} H={H}: verified {int((st >= 0).sum())}/{N} (checker {int((ds >= 0).sum())}), worst relative distance "
          f"{worst:.3e} at cond(H_FF) {worst_cond:.3e}")
    assert both.sum() >= 0.75 * N
    assert np.all(ro[st >= 0] <= TOL)


def _step_conds(I, H, th_i, nlt_i, seqs_i, states_i):
    """largest cond(H_FF) over the steps of one instance's loop"""
    worst = 1.0
    for k in range(seqs_i.shape[0]):
        rows = []
        for t in range(H):
            src, r = rd.target_source(H, k, t, nlt_i is not None)
            rows.append(th_i["targets"][r] if src == "targets" else nlt_i[r])
        tk = dict(th_i, x0=th_i["x0"] if k == 0 else states_i[k - 1], targets=np.array(rows))
        worst = max(worst, dense.instance(I, H, tk, seqs_i[k], np.zeros((H, I)))[2])
    return worst


@functools.lru_cache(maxsize=None)
def _recorded(I, H):
    """the oracle's closed loop at eps 1e-12, moved onto the stationary points of its own active sets by the dense
    closed loop (what tests/test_rollout_grad_host.py does), with the references' gradients"""
    th = _family(I, H, N)
    nlt = fm.new_last_targets(th, S, seed=H)
    rng = np.random.default_rng(5)
    G_u, G_x = rng.standard_normal((N, S, I)), rng.standard_normal((N, S, 2))
    refs, seqs, states, keep, conds = [], [], [], [], []
    for i in range(N):
        t0 = {k: th[k][i] for k in NAMES}
        _, _, sq, _ = rd.replay(I, H, S, t0, nlt[i], **TIGHT)
        ref, _, xs, psq = rd.closed_loop(I, H, S, t0, nlt[i], sq, G_u[i], G_x[i])
        keep.append(all(np.array_equal(dense.active(psq[k], t0["lo"], t0["hi"]), dense.active(sq[k], t0["lo"], t0["hi"]))
                        for k in range(S)))
        conds.append(_step_conds(I, H, t0, nlt[i], psq, xs))
        refs.append(ref); seqs.append(psq); states.append(xs)
    keep = np.array(keep)
    assert keep.sum() >= 0.75 * N, keep
    return th, nlt, G_u, G_x, refs, np.array(seqs), np.array(states), keep, np.array(conds)


@pytest.mark.parametrize("I,H", SHAPES)
def test_host_rollout_backward_and_forward_match_the_dense_closed_loop(I, H):
    th, nlt, G_u, G_x, refs, seqs, states, keep, conds = _recorded(I, H)
    dirs = td.random_tangents(I, H, S, N, 31 + H, K=1)
    tan = td.soa_tangents(dirs, N)
    io = dict(sequences=dense.soa(seqs, N), states=dense.soa(states, N), inputs=I)
    with MpcSolver(horizon=H, device=None) as s:
        out = s.rollout_backward(S, *_ins(th), dense.soa(nlt, N), grad_controls=dense.soa(G_u, N),
                                 grad_states=dense.soa(G_x, N), **io)
        assert s.last_flags == 0
        tu, tx = s.rollout_forward(S, *_ins(th), dense.soa(nlt, N), tangents=tan, **io)
        assert s.last_flags == 0
    worst, worst_cond = 0.0, 1.0
    for i in np.flatnonzero(keep):
        t0 = {k: th[k][i] for k in NAMES}
        for k in list(NAMES) + ["nlt"]:
            r = _held(out[KEY[k]][:, i], refs[i][k].ravel(), conds[i], f"instance {i} (class {i % 6}) d{k}", LOOP_FLOOR)
            if r > worst:
                worst, worst_cond = r, conds[i]
        wu, wx, _, _ = td.closed_loop_jvp(I, H, S, t0, nlt[i], seqs[i], {k: v[i] for k, v in dirs[0].items()})
        for got, want, what in ((tu[0][:, i], wu.ravel(), "tcontrols"), (tx[0][:, i], wx.ravel(), "tstates")):
            r = _held(got, want, conds[i], f"instance {i} (class {i % 6}) {what}")
            if r > worst:
                worst, worst_cond = r, conds[i]
    ident = float(mismatch([dense.soa(G_u, N) * tu[0], dense.soa(G_x, N) * tx[0]],
                           [out[k] * tan[k][0] for k in tan]).max())
    print(f"I={I} H={H} S={S}: kept {int(keep.sum())}/{N}, worst relative error {worst:.3e} at cond(H_FF) {worst_cond:.3e}, "
          f"transpose identity {ident:.3e} (bound {IDENTITY_BOUND:.3e})")
    assert ident <= IDENTITY_BOUND


@pytest.mark.parametrize("with_plant", [False, True], ids=["newton", "plant"])
@pytest.mark.parametrize("I,H", SHAPES)
def test_host_newton_and_plant_loops_match_the_dense_closed_loop(I, H, with_plant):
    """rollout_newton (FALLBACK_NONE) and rollout_plant (NEWTON, NONE) from a cold start: the instances carried through
    every step are the dense closed loop on their own active sets (controls and states), and the backward and forward
    entries at the checker's stationary loop give its gradients and its jvp -- the plant's and the disturbance's too."""
    th = _family(I, H, N)
    nlt = fm.new_last_targets(th, S, seed=H)
    ins, nl = _ins(th), dense.soa(nlt, N)
    plant = dist = pl = ds = None
    if with_plant:
        *plant, dist = fm.full_plant(th, PLANT_SCALE, steps=S)
        plant = tuple(plant)
        pl, ds = tuple(dense.soa(a, N) for a in plant), dense.soa(dist, N)
    with MpcSolver(horizon=H, device=None) as s:
        u, x, q, st, _, first = s.rollout_newton(S, *ins, nl, inputs=I, tol=TOL, max_rounds=ROUNDS, fallback="none",
                                              plant=pl, disturbance=ds)
    carried = np.flatnonzero(first == S)
    assert carried.size >= 0.75 * N, first
    seqs = np.ascontiguousarray(q.T).reshape(N, S, H, I)
    rng = np.random.default_rng(21 + H)
    G_u, G_x = rng.standard_normal((N, S, I)), rng.standard_normal((N, S, 2))
    dirs = td.random_tangents(I, H, S, N, 33 + H, K=1)
    extra = {}
    if with_plant:
        extra = dict(Ap=rng.standard_normal((N, 4)), Bp=rng.standard_normal((N, 2 * I)), Cp=rng.standard_normal((N, 2)),
                     d=rng.standard_normal((N, S, 2)))
    tan = td.soa_tangents(dirs, N)
    tan.update({KEY[k]: dense.soa(v, N)[None] for k, v in extra.items()})
    refs, psq, pxs, conds = {}, np.zeros((N, S, H, I)), np.zeros((N, S, 2)), {}
    worst, worst_cond = 0.0, 1.0
    for i in carried:
        t0 = {k: th[k][i] for k in NAMES}
        pi = None if plant is None else tuple(a[i] for a in plant)
        di = None if dist is None else dist[i]
        refs[i], pu, pxs[i], psq[i] = plant_dense.closed_loop(I, H, S, t0, nlt[i], seqs[i], G_u[i], G_x[i], pi, di)
        conds[i] = _step_conds(I, H, t0, nlt[i], psq[i], pxs[i])
        for got, want, what in ((u[:, i], pu.ravel(), "controls"), (x[:, i], pxs[i].ravel(), "states")):
            r = _held(got, want, conds[i], f"instance {i} (class {i % 6}) {what}")
            if r > worst:
                worst, worst_cond = r, conds[i]
    with MpcSolver(horizon=H, device=None) as s:
        io = dict(sequences=dense.soa(psq, N), states=dense.soa(pxs, N), inputs=I, plant=pl)
        out = s.rollout_backward(S, *ins, nl, grad_controls=dense.soa(G_u, N), grad_states=dense.soa(G_x, N),
                                 disturbance=ds, **io)
        tu, tx = s.rollout_forward(S, *ins, nl, tangents=tan, **io)
    names = list(NAMES) + ["nlt"] + (["Ap", "Bp", "Cp", "d"] if with_plant else [])
    for i in carried:
        t_i = dict({k: v[i] for k, v in dirs[0].items()}, **{k: v[i] for k, v in extra.items()})
        pi = None if plant is None else tuple(a[i] for a in plant)
        di = None if dist is None else dist[i]
        wu, wx, _, _ = plant_dense.closed_loop_jvp(I, H, S, {k: th[k][i] for k in NAMES}, nlt[i], psq[i], t_i, pi, di)
        pairs = [(out[KEY[k]][:, i], refs[i][k].ravel(), f"d{k}") for k in names]
        pairs += [(tu[0][:, i], wu.ravel(), "tcontrols"), (tx[0][:, i], wx.ravel(), "tstates")]
        for got, want, what in pairs:
            r = _held(got, want, conds[i], f"instance {i} (class {i % 6}) {what}", LOOP_FLOOR if what[0] == "d" else 0.0)
            if r > worst:
                worst, worst_cond = r, conds[i]
    print(f"I={I} H={H} S={S} plant={with_plant}: carried {carried.size}/{N}, worst relative error {worst:.3e} at "
          f"cond(H_FF) {worst_cond:.3e}")
