"""CPU side of tests/test_compact_loop_paths_gpu.py (no GPU): the compact closed loop's two entries on a host-only
handle OFF the default vehicle -- negative and zero speeds, T < 0, l < 0, weight_phi = 0, exchanged steering weights,
unequal and offset boxes (tests/model/vehicles.py) -- and the conditions the GPU module's inputs have to meet.

  - per cell (vehicle x H in 4, 5, 7, 20; n = 333, S = 4): both signs of v and v[3] = 0; 16 rounds carry at least 100
    instances to the end, instance 3 among them; 2 rounds carry at least 30 and stop at least 40.  The host path is
    deterministic: these are conditions on the inputs, printed per cell, not tolerances;
  - the forward, with and without x0, at both round counts: every row is tpc_mpc_rollout_newton's on the expanded
    arrays (compact_loop_common.reference) bit for bit, and the flags are equal; one cell per horizon with every
    speed negative;
  - the backward at the 16-round records with their status: the criteria of
    tests/test_compact_loop_grad_host.py::test_equals_the_general_backward_through_the_chain_rule on the carried
    instances, +0.0 on the others, flags 0;
  - subsets() is free of repeats and holds each layout pair; one_fallback_case() stops exactly instance 77; the batch
    of the GPU module's subset tests stops some but not all; the raw callers with a subset of the arrays give the
    all-arrays bytes on the host-only handle and leave everything else alone.

The central differences of the new vehicles are cells of test_compact_loop_grad_host.py."""
import numpy as np
import pytest

from tests.model import compact_grad_common as cg
from tests.model import compact_loop_common as cl
from tests.model import compact_loop_grad_common as lg
from tests.model import compact_loop_paths as cp
from trajectory_controller_amd import capi

CELLS = pytest.mark.parametrize("name,H", cp.cells())
X0 = pytest.mark.parametrize("with_x0", [False, True], ids=["x0=null", "x0"])


def test_there_are_35_cells():
    assert len(cp.cells()) == 35 and {H for _, H in cp.cells()} == set(cp.HORIZONS)
    assert ("short_fast", 20) not in cp.cells() and ("short_fast", 7) in cp.cells()


@CELLS
def test_the_cells_meet_what_the_gpu_criteria_rest_on(name, H):
    cs = cp.case(name, H)
    assert cs.n == 333 and (cs.v > 0).any() and (cs.v < 0).any() and cs.v[3] == 0.0
    for with_x0 in (False, True):
        full, short = cp.carried(cs, cp.ROUNDS_FULL, with_x0), cp.carried(cs, cp.ROUNDS_SHORT, with_x0)
        print(f"{name} H={H} x0={with_x0}: {cp.ROUNDS_FULL} rounds carry {int(full.sum())}/{cs.n}, {cp.ROUNDS_SHORT} "
              f"rounds carry {int(short.sum())} and stop {int((~short).sum())}")
        assert full.sum() >= 100 and full[3]
        assert short.sum() >= 30 and (~short).sum() >= 40


def _forward_equals_the_reference(cs, with_x0, rounds):
    mine = cp.host_forward(cs, rounds, with_x0)
    with cp.host_solver(cs) as s:
        ref = cl.reference(s, cs.S, cs.v, cs.dy, cs.dphi, cs.x0 if with_x0 else None, tol=cp.TOL, rounds=rounds)
    assert cl.same_rows(dict(mine, first=mine["first"][0]), ref) == []
    assert mine["flags"] == ref["flags"]
    return mine


@pytest.mark.parametrize("rounds", [cp.ROUNDS_FULL, cp.ROUNDS_SHORT])
@X0
@CELLS
def test_forward_equals_rollout_newton_on_the_expanded_arrays(name, H, with_x0, rounds):
    _forward_equals_the_reference(cp.case(name, H), with_x0, rounds)


@pytest.mark.parametrize("rounds", [cp.ROUNDS_FULL, cp.ROUNDS_SHORT])
@pytest.mark.parametrize("H", cp.HORIZONS)
def test_forward_with_every_speed_negative(H, rounds):
    cs = cp.case("asym", H, reverse_only=True)
    assert np.all(cs.v < 0)
    mine = _forward_equals_the_reference(cs, True, rounds)
    assert rounds != cp.ROUNDS_FULL or (mine["first"][0] == cs.S).sum() >= 100


@X0
@CELLS
def test_backward_equals_the_general_backward_through_the_chain_rule(name, H, with_x0):
    cs = cp.case(name, H)
    rec = cp.host_forward(cs, cp.ROUNDS_FULL, with_x0)
    ok = (rec["status"] >= 0).all(axis=0)
    assert np.array_equal(ok, cp.carried(cs, cp.ROUNDS_FULL, with_x0))
    x0 = cs.x0 if with_x0 else None
    gc, gs = cp.grads(cs)
    got = cp.host_backward(cs, cp.ROUNDS_FULL, with_x0)
    with cp.host_solver(cs) as s:
        ref, d, rflags = lg.reference(s, cs.S, H, cs.v, cs.dy, cs.dphi, x0, rec["sequences"], rec["states"], gc, gs)
        ty, tp = lg.target_terms(s, cs.S, H, cs.v, cs.dy, cs.dphi, x0, rec["sequences"], rec["states"], gc, gs)
    assert got["flags"] == 0 and rflags == 0
    for k in lg.PER_INSTANCE:
        assert not cl.bits(got[k][..., ~ok]).any(), k           # excluded by their status: +0.0
    for k in lg.EXACT:
        mine = got[k].reshape(np.shape(ref[k]))
        assert cg.same_numbers(mine[..., ok], ref[k][..., ok]), k
    assert np.isfinite(got["params"]).all()
    assert got["params"].tobytes() == lg.ascending(got["params_rows"]).tobytes()
    for key, terms, rows in (("delta_y", ty, d["targets"][0::2]), ("delta_phi", tp, d["targets"][1::2])):
        exact, bound = lg.fsum_cols(rows), lg.target_bound(terms)
        diff, own = np.abs(got[key][0] - exact), np.abs(lg.fsum_cols(terms) - exact)
        scale = np.maximum(bound, 1e-300)
        print(f"{name} H={H} {key}: max |got - fsum(reference rows)| / bound {np.max((diff / scale)[ok]):.3f}, "
              f"max |fsum(terms) - fsum(reference rows)| / bound {np.max((own / scale)[ok]):.3f}")
        assert np.all(own[ok] <= bound[ok]), key       # the terms are the reference's: the bound itself is checked
        assert np.all(diff[ok] <= bound[ok]), key


def test_subsets_are_free_of_repeats_and_hold_each_layout_pair():
    fwd, bwd = cp.subsets("forward"), cp.subsets("backward")
    for subs, opt in ((fwd, cp.FWD_OPTIONAL), (bwd, cp.BWD_OUTPUTS)):
        assert len(set(subs)) == len(subs)
        assert frozenset() in subs and frozenset(opt) in subs
        for k in opt:
            assert frozenset(opt) - {k} in subs and frozenset({k}) in subs
    # the fallback's batch: "a missing, b present", the rest of the batch's rows missing, first_unverified present.
    # {status, first}: the status rows at int32 row 0 with no fp64 output row but the controls' in front
    for a, b in zip(cp.FALLBACK_ORDER, cp.FALLBACK_ORDER[1:]):
        assert frozenset({b, "first"}) in fwd, (a, b)
    # the staging table holds every optional array: its pairs are the arrays alone
    for a, b in zip(cp.STAGE_ORDER, cp.STAGE_ORDER[1:]):
        assert cp.layout_pair("forward", cp.STAGE_ORDER, b) == frozenset({b}) and frozenset({b}) in fwd, (a, b)
    assert len(fwd) == 18 and len(bwd) == 16


@pytest.mark.parametrize("H", [4, 7])
def test_the_batch_of_one_fallback(H):
    cs = cp.one_fallback_case(H)
    first = cp.host_forward(cs, cp.ROUNDS_SHORT, True)["first"][0]
    assert cs.n == 130 and np.flatnonzero(first < cs.S).tolist() == [cp.ONE_AT]


@pytest.mark.parametrize("H", [4, 7])
def test_raw_callers_with_subsets_on_the_host_only_handle(H):
    """the GPU module's subset batch (asym, n = 130, S = 3): some instances stop, not all; and what that module asserts
    of a device holds on the host-only handle"""
    cs, lib = cp.case("asym", H, 130, 3), capi.load_library()
    stopped = int((~cp.carried(cs, cp.ROUNDS_SHORT, True)).sum())
    print(f"asym H={H} n=130 S=3: {cp.ROUNDS_SHORT} rounds stop {stopped}, {cp.ROUNDS_FULL} rounds stop "
          f"{int((~cp.carried(cs, cp.ROUNDS_FULL, True)).sum())}")
    assert 1 <= stopped <= 129
    rec = cp.host_forward(cs, cp.ROUNDS_FULL, True)
    gc, gs = cp.grads(cs)
    with cp.host_solver(cs) as hs:
        for present in cp.subsets("forward"):
            res = cp.run_forward(lib, hs, cs, cp.mem_of(cs), present)
            cp.check_forward(cp.host_forward(cs, cp.ROUNDS_SHORT, True), *res)
        for want in cp.subsets("backward"):
            res = cp.run_backward(lib, hs, cs, cp.mem_of(cs), want, rec["sequences"], rec["states"], rec["status"],
                                  gc, gs)
            assert set(res[2]) == set(want)
            cp.check_backward(cp.host_backward(cs, cp.ROUNDS_FULL, True), *res, device=False)
