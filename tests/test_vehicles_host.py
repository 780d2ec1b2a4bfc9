"""CPU tests of the compact-form vehicle family (tests/model/vehicles.py): what tests/test_vehicles_gpu.py's criteria
rest on, re-measured here, and the one place where the LANE_FMA arithmetic leaves dlib's path off the default vehicle.

Cells: vehicle x horizon, n = 600 up to N = 20 and 200 above; the GPU module's batches (333 / 141) are prefixes of
them, and every condition is asserted on the prefix too.  Conditions: both signs of v and one v == 0 in every cell; the
oracle's share of capped instances <= 0.15; a median iteration count >= 60 (the solves are long enough to go wrong)
-- except `offset`, whose box does not contain u = 0: the cold start is clamped onto a corner and most instances
end there at once (median 0 to 2, measured); it is in the family for the exact stop-test build and the clamp, and
its cells hold >= 5 % of instances beyond the coordinate-descent phase, which is asserted instead.  UbModel
(fast_stop=None: the build the kernels' screens choose) has the oracle's iteration counts and |du| <= 1e-9 in every
cell but (no_phi, N = 5).

The finding (NOTEBOOK.md, "A tie in dlib's arg-max").  weight_phi = 0, N = 5, reversing at |T v| in 0.21 .. 0.31: the
coordinate-descent phase reaches a gradient whose three largest components are ONE real number (a structural tie, not a
coincidence of the inputs), dlib's strict '>' and the family's rounding pick different winners, both valid descent
steps, and the two solves part: 65 of 3000 counts differ on the batch below (82 paths), |du| up to 1.3e-3.  Both answers pass
dlib's own stop test, evaluated densely in fp64 on the returned sequences.  AUTO sends such requests to the bit-exact
kernels (csrc/tpc_mpc_api.cpp, cd_tie_prone: weight_phi <= 2^-30 weight_y); a host-only handle has none and keeps the
family's answer."""
import functools

import numpy as np
import pytest

from conftest import bits_equal
from oracle.bindings import Oracle
from tests.model import mpc_polish_dense as pd
from tests.model import vehicles as vh
from tests.model.bindings import UbModel
from tests.model.compact_exact_common import NAMES, expand
from trajectory_controller_amd import MpcSolver

NTHREADS = 8
ATOL = 1e-9
CAP = 10000
FINDING = ("no_phi", 5)
# instances of a finding batch whose iteration count is not the oracle's -- measured on the CPU, asserted exactly
TIE_MIXED_600 = 6            # the family's own (no_phi, 5) cell, n = 600
# reverse_only, n = 3000, first = 31000: (counts differ, counts differ or |du| > 1e-9 -- some paths part and end after the
# same number of iterations)
TIE_REVERSED = {"no_phi": (56, 69), "default_no_phi": (65, 82)}


def _n(H):
    return 600 if H <= 20 else 200


@functools.lru_cache(maxsize=None)
def _cell(name, H):
    """oracle and model on one cell, shared by the tests (never modified)"""
    v, dy, dphi = vh.inputs(H, _n(H))
    kw = vh.oracle_kw(name)
    of, orr, oit = Oracle().solve_compact(H, v, dy, dphi, nthreads=NTHREADS, **kw)
    mf, mr, mit, mfl = UbModel().solve_compact(H, v, dy, dphi, nthreads=NTHREADS, fast_stop=None, **kw)
    return dict(v=v, dy=dy, dphi=dphi, of=of, orr=orr, oit=oit, mf=mf, mr=mr, mit=mit, mfl=mfl)


def test_the_table_is_the_documented_one():
    assert vh.NAMES == ("default", "long_slow", "short_fast", "rear_cheap", "neg_l", "neg_T", "no_phi", "asym", "offset")
    assert vh.VEHICLES["default"] == ((20.0, 7.0, 0.0005, 10.0), 0.1, 0.21, (-vh.A22, -vh.A22), (vh.A22, vh.A22))
    assert vh.VEHICLES["neg_l"][2] < 0 and vh.VEHICLES["neg_T"][1] < 0 and vh.VEHICLES["no_phi"][0][1] == 0
    lo, hi = vh.VEHICLES["asym"][3:]
    assert lo[0] != lo[1] and hi[0] != hi[1] and hi[0] - lo[0] != hi[1] - lo[1]      # s0 != s1, dlt != 0
    lo, hi = vh.VEHICLES["offset"][3:]
    assert lo[0] > 0 and hi[1] < 0                                                   # u = 0 outside the box
    assert len(vh.cells()) == 9 * 3 + 8 * 3 and ("short_fast", 20) not in vh.cells()
    # a batch is a prefix of every longer one, and reverse_only reverses every speed
    a, b = vh.inputs(20, 141), vh.inputs(20, 600)
    assert all(bits_equal(x, y[:141]) for x, y in zip(a, b))
    assert np.all(vh.inputs(5, 100, reverse_only=True)[0] < 0)


@pytest.mark.parametrize("name,H", vh.cells())
def test_cell_conditions(name, H):
    c = _cell(name, H)
    for m in (_n(H), vh.batch_size(H)):
        v, oit = c["v"][:m], c["oit"][:m]
        neg, pos = float(np.mean(v < 0)), float(np.mean(v > 0))
        capped, med = float(np.mean(oit >= CAP)), float(np.median(oit))
        print(f"{name} H={H} n={m}: v<0 {neg:.3f}, capped {capped:.3f}, median iterations {med:.0f}")
        assert 0.2 <= neg <= 0.4 and pos >= 0.6 and v[3] == 0
        assert capped <= 0.15
        if name == "offset":
            assert float(np.mean(oit > 50)) >= 0.05
        else:
            assert med >= 60


@pytest.mark.parametrize("name,H", vh.cells())
def test_model_follows_the_oracle(name, H):
    c = _cell(name, H)
    err = np.maximum(np.abs(c["mf"] - c["of"]), np.abs(c["mr"] - c["orr"]))
    differ = c["mit"] != c["oit"]
    print(f"{name} H={H}: max |du| {err.max():.2e}, counts differ in {int(differ.sum())} of {_n(H)}")
    if (name, H) == FINDING:
        assert int(differ.sum()) == TIE_MIXED_600
        assert np.all(c["v"][differ] < 0)
        assert err[~differ].max() <= ATOL
        assert not differ[:vh.batch_size(H)].all()
        return
    assert not differ.any()
    assert err.max() <= ATOL
    # a control dlib leaves on a bound is on it bit for bit
    lo, hi = vh.VEHICLES[name][3:]
    for j, (o, m) in enumerate(((c["of"], c["mf"]), (c["orr"], c["mr"]))):
        assert np.array_equal((o == lo[j]) | (o == hi[j]), (m == lo[j]) | (m == hi[j]))


@pytest.mark.parametrize("name,H", vh.cells())
def test_ties_are_in_one_cell_only(name, H):
    """vehicles.cd_ties (dense numpy, no solver under test): no cell but (no_phi, 5) meets a tied arg-max, so the GPU
    module may hold every tolerance family to the oracle's counts everywhere else; in that cell 13 of 600 instances tie
    (5 of the GPU batch's 333), and every instance on which the model leaves dlib's path is one of them."""
    c = _cell(name, H)
    ties = vh.cd_ties(name, H, c["v"], c["dy"], c["dphi"])
    if (name, H) != FINDING:
        assert not ties.any()
        return
    differ = c["mit"] != c["oit"]
    assert int(ties.sum()) == 13 and int(ties[:vh.batch_size(H)].sum()) == 5
    assert np.all(ties[differ]) and np.all(c["v"][ties] < 0)


@pytest.mark.parametrize("name", ["offset", "asym", "default"])
def test_the_screens_choose_the_documented_build(name):
    """`offset` fails fast_stop_ok (u = 0 outside the box) and takes the exact stop-test build; the others the fast one:
    fast_stop=None equals the build named, bit for bit."""
    H = 10
    v, dy, dphi = vh.inputs(H, 200)
    kw = vh.oracle_kw(name)
    m = UbModel()
    auto = m.solve_compact(H, v, dy, dphi, nthreads=NTHREADS, fast_stop=None, **kw)
    named = m.solve_compact(H, v, dy, dphi, nthreads=NTHREADS, fast_stop=name != "offset", **kw)
    assert bits_equal(auto[0], named[0]) and bits_equal(auto[1], named[1]) and np.array_equal(auto[2], named[2])


@pytest.mark.parametrize("H", [4, 5, 20])
@pytest.mark.parametrize("name", ["neg_l", "asym", "rear_cheap"])
def test_host_solve_one_is_the_model(name, H):
    """tpc_mpc_solve_one on a host-only handle: UbModel's bits, the oracle's iteration counts (24 inputs, both signs)."""
    c = _cell(name, H)
    k = 24
    assert (c["v"][:k] < 0).any() and (c["v"][:k] > 0).any()
    with MpcSolver(horizon=H, device=None, **vh.solver_kw(name)) as s:
        for i in range(k):
            f, r = s.solve_one(float(c["v"][i]), float(c["dy"][i]), float(c["dphi"][i]))
            _, it = s.last_solve_one_flags()
            assert bits_equal([f, r], [c["mf"][i], c["mr"][i]]), i
            assert it == c["oit"][i] == c["mit"][i], i


# ---------------------------------------------------------------------------------------------
# the tie

def _masked_gradient(H, th, k, seq):
    """dlib's stop quantity (mpc.h:289-311) of instance k at the sequence seq [H, 2], dense fp64: max |df| over the
    variables that are not blocked on a bound"""
    one = {key: th[key][:, k].reshape(-1) for key in NAMES}
    one["targets"] = one["targets"].reshape(H, 2)
    Hs, MM, lo, hi = pd.problem(2, H, one)
    u = np.asarray(seq, dtype=np.float64).reshape(-1)
    df = pd.gradient(Hs, MM, u)
    return pd.residual(df, pd.free_set(df, u, lo, hi))


@functools.lru_cache(maxsize=None)
def _reversed(which):
    H, n = 5, 3000
    v, dy, dphi = vh.inputs(H, n, reverse_only=True, first=31000)
    kw = vh.oracle_kw("no_phi") if which == "no_phi" else dict(weights=(20.0, 0.0, 0.0005, 10.0))
    skw = vh.solver_kw("no_phi") if which == "no_phi" else dict(weight_phi=0.0)
    of, orr, oit = Oracle().solve_compact(H, v, dy, dphi, nthreads=NTHREADS, **kw)
    mf, mr, mit, _, seq = UbModel().solve_compact(H, v, dy, dphi, nthreads=NTHREADS, fast_stop=None,
                                                  want_sequence=True, **kw)
    return dict(H=H, v=v, dy=dy, dphi=dphi, of=of, orr=orr, oit=oit, mf=mf, mr=mr, mit=mit, seq=seq, kw=kw, skw=skw)


@pytest.mark.parametrize("which", list(TIE_REVERSED))
def test_tie_share_and_both_answers_stop_dlibs_test(which):
    """Reversing, weight_phi = 0, N = 5 (`default_no_phi`: the default vehicle's T, l and box with weights 20 / 0 /
    0.0005 / 10).  The share that leaves dlib's path (another count, or |du| > 1e-9) is the measured one; and the
    sequence the family returns -- on EVERY such instance -- is an answer by dlib's own test: the dense
    fp64 masked gradient there is below eps.  (The oracle's own sequence passes the same evaluation: the check's
    control.)"""
    c = _reversed(which)
    H = c["H"]
    err = np.maximum(np.abs(c["mf"] - c["of"]), np.abs(c["mr"] - c["orr"]))
    counts = c["mit"] != c["oit"]
    differ = counts | (err > ATOL)
    print(f"{which}: counts differ in {int(counts.sum())}, paths in {int(differ.sum())} of {len(differ)}, max |du| {err.max():.2e} "
          f"(elsewhere {err[~differ].max():.2e}), |T v| of the differing "
          f"{np.abs(c['kw'].get('T', 0.1) * c['v'][differ]).min():.3f} .. {np.abs(c['kw'].get('T', 0.1) * c['v'][differ]).max():.3f}")
    assert (int(counts.sum()), int(differ.sum())) == TIE_REVERSED[which]
    assert bits_equal(c["seq"][:, 0, 0], c["mf"]) and bits_equal(c["seq"][:, 0, 1], c["mr"])
    with MpcSolver(horizon=H, device=None, **c["skw"]) as s:
        th = expand(s.params, H, c["v"], c["dy"], c["dphi"])
    eps, worst = 0.01, 0.0
    for k in np.flatnonzero(differ):
        g = _masked_gradient(H, th, k, c["seq"][k])
        worst = max(worst, g)
        assert g < eps, (k, g)
    print(f"{which}: dense masked gradient at the family's sequences of the differing instances: max {worst:.3e} < eps {eps}")
    # control: the oracle's own sequences under the same evaluation
    g = {key: np.ascontiguousarray(th[key].T) for key in NAMES}
    ks = np.flatnonzero(differ)[:16]
    _, controls, _ = Oracle().solve_general(2, H, *[g[key][ks] for key in ("A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets")])
    assert bits_equal(controls[:, 0, 0], c["of"][ks])
    for j, k in enumerate(ks):
        assert _masked_gradient(H, th, k, controls[j]) < eps


def test_tie_needs_the_reversal_the_horizon_and_weight_phi_zero():
    """+v, N = 4 / 10 / 20, and weight_phi = 1e-3 on the same inputs: the model has the oracle's counts everywhere."""
    m, o = UbModel(), Oracle()
    base = vh.oracle_kw("no_phi")
    for H, rev, wphi in ((5, False, 0.0), (4, True, 0.0), (10, True, 0.0), (20, True, 0.0), (5, True, 1e-3)):
        v, dy, dphi = vh.inputs(H, 1000, reverse_only=True, first=31000)
        kw = dict(base, weights=(20.0, wphi, 0.0005, 10.0))
        v = v if rev else -v
        of, orr, oit = o.solve_compact(H, v, dy, dphi, nthreads=NTHREADS, **kw)
        mf, mr, mit, _ = m.solve_compact(H, v, dy, dphi, nthreads=NTHREADS, fast_stop=None, **kw)
        assert np.array_equal(mit, oit), (H, rev, wphi)
        assert max(np.abs(mf - of).max(), np.abs(mr - orr).max()) <= ATOL, (H, rev, wphi)


def test_tie_is_structural():
    """The cause, on the traced instance (v = -3.8658..., T = 0.07, l = 0.26, N = 5): after dlib's coordinate steps on
    u[0](1), u[0](1), u[0](0) the dense gradient has df[1](0) == df[2](0) == -df[2](1) to rounding (relative 1e-13,
    against 1e-2 for the next component), and they are the largest free components -- the arg-max is decided by the
    last bits.  Dense fp64, independent of both solvers."""
    H = 5
    v, dy, dphi = np.array([-3.865858607583298]), np.array([-0.38772990577606214]), np.array([0.4298939292625942])
    with MpcSolver(horizon=H, device=None, **vh.solver_kw("no_phi")) as s:
        th = expand(s.params, H, v, dy, dphi)
    one = {key: th[key][:, 0].reshape(-1) for key in NAMES}
    one["targets"] = one["targets"].reshape(H, 2)
    Hs, MM, lo, hi = pd.problem(2, H, one)
    Hs, MM = np.asarray(Hs), np.asarray(MM)
    R = np.tile(np.asarray(vh.VEHICLES["no_phi"][0][2:]), H)
    u = np.zeros(2 * H)
    picks = []
    for _ in range(3):
        df = Hs @ u + MM
        free = pd.free_set(df, u, lo, hi)
        best = int(np.argmax(np.where(free, np.abs(df), 0.0)))
        picks.append(best)
        qd = Hs[best, best] - R[best]                       # dlib's Q_diag leaves R out (mpc.h:116-123, :324)
        u[best] = np.clip(-(df[best] - qd * u[best]) / qd, lo[best], hi[best])
    assert picks == [1, 1, 0]                               # (step, input) = (0, 1), (0, 1), (0, 0)
    df = Hs @ u + MM
    mag = np.sort(np.abs(df))[::-1]
    three = np.array([df[2 * 1 + 0], df[2 * 2 + 0], -df[2 * 2 + 1]])
    assert np.all(np.abs(three - three[0]) <= 1e-12 * abs(three[0]))
    assert abs(abs(three[0]) - mag[0]) <= 1e-12 * mag[0] and mag[3] < 0.99 * mag[0]


# ---------------------------------------------------------------------------------------------
# the exact compact entries off the default vehicle

EXACT_N, EXACT_K = 97, 2


def exact_entries(name, H, device, torch=None):
    """solve_batch_compact_exact (fallback none), its backward and its forward mode on the first 97 instances of a cell,
    on a host-only handle (device=None) or a device handle fed numpy arrays (torch=None) or CUDA tensors: every
    per-instance output as numpy, by name.  Shared with tests/test_vehicles_gpu.py, which holds the device to these."""
    from tests.model import compact_grad_common as cg
    from tests.model import compact_tangent_common as ct
    v, dy, dphi = vh.inputs(H, EXACT_N)
    assert (v < 0).sum() >= 20 and (v > 0).sum() >= 20
    gf, gr, gs = cg.grad_in(H, EXACT_N, 77 + H, sequence=True)
    d = ct.directions(EXACT_N, EXACT_K, 78 + H)
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")) if torch is not None else (lambda a: a)
    down = lambda a: np.ascontiguousarray(a.cpu().numpy() if torch is not None else a)
    with MpcSolver(horizon=H, device=device, **vh.solver_kw(name)) as s:
        tv, ty, tp = up(v), up(dy), up(dphi)
        front, rear, seq, st, _, rin, rout = s.solve_batch_compact_exact(tv, ty, tp, fallback="none", want_sequence=True,
                                                                         want_residuals=True)
        out = dict(front=down(front), rear=down(rear), sequence=down(seq), status=down(st), residual_in=down(rin))
        ok = out["status"] >= 0
        out["residual_out"] = np.where(ok, down(rout), 0.0)
        g = s.solve_batch_compact_exact_backward(tv, ty, tp, seq, up(gf), up(gr), up(gs), status=st,
                                                 want=cg.PER_INSTANCE + ("params",))
        for k in cg.PER_INSTANCE:
            out["d" + k] = down(g[k])
        out["dparams_is_the_device_sum"] = np.array(
            device is None or down(g["params"]).tobytes() == cg.device_sum(out["dparams_rows"]).tobytes())
        tf, tr, tseq = s.solve_batch_compact_exact_forward(tv, ty, tp, seq, {k: up(a) for k, a in d.items()}, status=st,
                                                           want_sequence=True)
        out.update(tfront=down(tf), trear=down(tr), tsequence=down(tseq))
    return out


@pytest.mark.parametrize("H", [5, 20])
@pytest.mark.parametrize("name", ["neg_l", "asym"])
def test_exact_compact_entries_are_the_general_ones_on_the_expanded_arrays(name, H):
    """tests/test_compact_exact_host.py, test_compact_grad_host.py and test_compact_tangent_host.py's statements with
    a negative wheelbase / unequal bounds and both signs of v: the solve is the polish of the expanded arrays from zero
    controls bit for bit; the backward pass and the forward mode equal, as numbers, the general entries on the expanded
    arrays pushed through the chain rule of the model building."""
    from tests.model import compact_grad_common as cg
    from tests.model import compact_tangent_common as ct
    from tests.model.compact_exact_common import bits
    c = exact_entries(name, H, None)
    v, dy, dphi = vh.inputs(H, EXACT_N)
    ok = c["status"] >= 0
    print(f"{name} H={H}: verified {int(ok.sum())}/{EXACT_N}")
    assert ok.sum() >= EXACT_N // 2 and ok[v < 0].any() and ok[v > 0].any()
    gf, gr, gs = cg.grad_in(H, EXACT_N, 77 + H, sequence=True)
    d = ct.directions(EXACT_N, EXACT_K, 78 + H)
    with MpcSolver(horizon=H, device=None, **vh.solver_kw(name)) as s:
        p = s.params
        th = expand(p, H, v, dy, dphi)
        u = np.zeros((2 * H, EXACT_N))
        _, pst, prin, prout = s.polish_batch_general(*[th[k] for k in NAMES], u, tol=1e-9, max_rounds=16, inputs=2)
        ref, rflags = cg.reference(s, H, v, dy, dphi, c["sequence"], gf, gr, gs)
        tref, tflags = ct.reference(s, th, p.step_size, p.wheelbase, H, v, c["sequence"], d, EXACT_K)
    assert np.array_equal(c["status"], pst) and np.array_equal(bits(c["sequence"]), bits(u))
    assert np.array_equal(bits(c["front"]), bits(u[0])) and np.array_equal(bits(c["rear"]), bits(u[1]))
    assert np.array_equal(bits(c["residual_in"]), bits(prin)) and np.array_equal(bits(c["residual_out"][ok]), bits(prout[ok]))
    assert rflags == 0 and tflags == 0
    for k in cg.PER_INSTANCE:
        assert cg.same_numbers(c["d" + k][..., ok], ref[k][..., ok]), k
        assert not np.any(c["d" + k][..., ~ok]), k
    assert ct.same_numbers(c["tfront"][:, ok], tref[:, 0][:, ok]) and ct.same_numbers(c["trear"][:, ok], tref[:, 1][:, ok])
    assert ct.same_numbers(c["tsequence"][..., ok], tref[..., ok])
    assert np.abs(tref[:, 0]).max() > 0 and np.abs(c["dv"]).max() > 0


# two instances of (no_phi, N = 5) on which the model leaves dlib's path: the one traced in NOTEBOOK.md (108 iterations
# against dlib's 109, front on its bound either way) and instance 1183 of the all-reversed batch, the largest |du| of
# that batch (1.24e-3; 100 iterations against 168)
TRACED = (-3.865858607583298, -0.38772990577606214, 0.4298939292625942)
PARTED = (-3.791436349261393, 0.4016942525532955, -0.37880874572147216)


def test_host_only_handle_keeps_the_model_answer_on_the_traced_tie():
    """The traced instance and the most parted one: the model leaves dlib's path there (another count), and a
    host-only handle, which has no bit-exact kernels to send the request to, answers with the model's bits under AUTO
    as include/tpc_mpc.h says.  (A GPU handle answers with dlib's: tests/test_vehicles_gpu.py.)"""
    H = 5
    kw = vh.oracle_kw("no_phi")
    with MpcSolver(horizon=H, device=None, algo="auto", **vh.solver_kw("no_phi")) as s:
        for (v, dy, dphi), apart in ((TRACED, 0.0), (PARTED, 1e-3)):
            of, orr, oit = Oracle().solve_compact(H, [v], [dy], [dphi], **kw)
            mf, mr, mit, _ = UbModel().solve_compact(H, [v], [dy], [dphi], fast_stop=None, **kw)
            assert mit[0] != oit[0] and max(abs(mf[0] - of[0]), abs(mr[0] - orr[0])) >= apart
            f, r = s.solve_one(v, dy, dphi)
            assert bits_equal([f, r], [mf[0], mr[0]]) and s.last_solve_one_flags() == (0, int(mit[0]))


@pytest.mark.parametrize("ratio,parted", [(5e-22, (65, 82)), (1e-16, (55, 65)), (1e-14, (1, 1)), (1e-12, (0, 0)),
                                           (2.0 ** -30, (0, 0)), (1e-6, (0, 0))])
def test_how_small_a_weight_phi_still_ties(ratio, parted):
    """What cd_tie_prone's threshold (weight_phi <= 2^-30 weight_y, csrc/tpc_mpc_api.cpp) rests on: on the all-reversed
    batch with the default vehicle's T, l and box, the solves that leave dlib's path (counts, paths) by weight_phi /
    weight_y.  A ratio of 5e-22 ties exactly like 0; nothing shows from 1e-12 on, three decades below the threshold."""
    c = _reversed("default_no_phi")
    kw = dict(weights=(20.0, 20.0 * ratio, 0.0005, 10.0))
    of, orr, oit = Oracle().solve_compact(5, c["v"], c["dy"], c["dphi"], nthreads=NTHREADS, **kw)
    mf, mr, mit, _ = UbModel().solve_compact(5, c["v"], c["dy"], c["dphi"], nthreads=NTHREADS, fast_stop=None, **kw)
    err = np.maximum(np.abs(mf - of), np.abs(mr - orr))
    counts = mit != oit
    assert (int(counts.sum()), int((counts | (err > ATOL)).sum())) == parted
