"""CPU side of tests/test_rollout_device_paths_gpu.py (no GPU): the conditions that module's inputs have to meet, asserted
through the host-only handle, and the shared helpers (tests/model/rollout_device_paths.py) checked against what exists.

  - the subsets of optional arrays are the ones the GPU module's docstring lists, without repeats;
  - for every batch and every set of optional inputs a FALLBACK_SOLVE call of the GPU module gets, the FALLBACK_NONE
    pass on the host predicts a fallback set (first_unverified < steps) that is not empty, not the whole batch and not a
    multiple of 64 in size; one_fallback_case() predicts exactly instance 77 in every mode;
  - the wide layout (ld = n + 13, the batch at column 5, ld_d = n + 29 or 0) gives the packed call's bytes on the
    host-only handle and leaves the padding alone, for the Newton loop, both backwards and every forward;
  - solve_loop without a plant from a zero start is mpc_rollout_polish_ref.replay, bit for bit."""
import numpy as np
import pytest

from tests.model import mpc_rollout_dense as rd
from tests.model import mpc_rollout_polish_ref as rp
from tests.model import rollout_device_paths as dp
from trajectory_controller_amd import MpcSolver, capi

BIG = [s for s in dp.SHAPES if s[3] > 64]


def test_subsets_are_what_the_issue_lists():
    for kind, opt in dp.LOOP_OPTIONAL.items():
        for mode in dp.MODES:
            subs = dp.subsets(kind, mode)
            assert len(set(subs)) == len(subs)
            assert frozenset() in subs and frozenset(opt) in subs
            for k in opt:
                assert frozenset(opt) - {k} in subs and frozenset({k}) in subs
    # the pairs "first missing, second present" of the two layouts, all other members of the layout missing
    newton = dp.subsets("newton", "both")
    rest = {"iters", "first", "c", "v"}
    for a, b in (("sequences", "status"), ("status", "rin"), ("rin", "rout")):
        assert frozenset(rest | {"states", "nlt", b}) in newton, (a, b)
    assert frozenset(rest | {"states", "nlt"}) in newton                       # rout missing, the disturbance present
    for a, b in (("nlt", "states"), ("states", "sequences"), ("sequences", "rin"), ("rin", "rout")):
        assert frozenset(rest | {"status", b}) in newton, (a, b)
    assert frozenset(rest | {"status"}) in newton
    assert len(newton) == 31 and len(dp.subsets("newton", None)) == 29
    assert len(dp.subsets("polished", None)) == 27 and len(dp.subsets("rollout", None)) == 12


def _given_sets(kind):
    return sorted({dp.given_inputs(s) for s in dp.subsets(kind, "both")}, key=sorted)


@pytest.mark.parametrize("mode", dp.MODES, ids=str)
@pytest.mark.parametrize("shape", BIG, ids=str)
def test_predicted_fallback_sets_end_in_a_partly_live_wavefront(shape, mode):
    cs = dp.case(*shape)
    gs = _given_sets("newton")
    assert len(gs) == 8          # every combination of controls_inout, v_inout and new_last_targets occurs
    for given in gs:
        first = dp.ref_loop(cs, "newton", mode, "none", given)["first"][0]
        count = int((first < cs.S).sum())
        print(f"{shape} {mode} {sorted(given)}: {count} of {cs.n} fall back")
        assert 0 < count < cs.n and count % 64 != 0, (sorted(given), count)


def test_the_batch_of_one_fallback():
    cs = dp.one_fallback_case()
    assert cs.n == 130 and not cs.c0.any()
    for mode in dp.MODES:
        for given in _given_sets("newton"):
            first = dp.ref_loop(cs, "newton", mode, "none", given)["first"][0]
            assert np.flatnonzero(first < cs.S).tolist() == [dp.ONE_AT], (mode, sorted(given))


@pytest.mark.parametrize("mode", dp.MODES, ids=str)
@pytest.mark.parametrize("shape", dp.SHAPES, ids=str)
def test_wide_arrays_give_the_packed_bytes_on_the_host_only_handle(shape, mode):
    cs = dp.case(*shape)
    lib = capi.load_library()
    with MpcSolver(horizon=cs.H, device=None) as hs:
        for present in (frozenset(dp.LOOP_OPTIONAL["newton"]), frozenset({"rin", "nlt"}), frozenset({"c"})):
            res = dp.run_loop(lib, hs, cs, dp.wide(cs.n, False), "newton", mode, "none", present)
            dp.check_loop(cs, "newton", mode, "none", present, *res)
        for zero in ((False, True) if mode is not None else (False,)):
            outs = dp.grad_outputs(mode)
            res = dp.run_backward(lib, hs, cs, dp.wide(cs.n, False), mode, outs, ld_d_zero=zero)
            dp.check_backward(cs, mode, *res)
            for K in (1, 3):
                names = dp.tangent_names(mode)
                res = dp.run_forward(lib, hs, cs, dp.wide(cs.n, False), mode, K, names, ld_d_zero=zero)
                dp.check_forward(cs, mode, K, names, False, *res)
        if mode is None:
            names = dp.tangent_names(None, single=True)
            res = dp.run_forward(lib, hs, cs, dp.wide(cs.n, False), None, 3, names, single=True)
            dp.check_forward(cs, None, 3, names, True, *res)


@pytest.mark.parametrize("shape", dp.SHAPES, ids=str)
@pytest.mark.parametrize("polished", [False, True], ids=["record", "polished"])
def test_solve_loop_is_the_polished_replay(shape, polished):
    cs = dp.case(*shape)
    I, H, S, n = shape
    th = {k: np.ascontiguousarray(a.T) for k, a in zip(rd.NAMES, cs.ins)}
    nlt = np.ascontiguousarray(cs.nl.T).reshape(n, S, 2)
    u0, xs, sq, st, it, ri, ro = rp.replay(I, H, S, th, nlt, tol=dp.TOL, max_rounds=dp.ROUNDS,
                                           polisher="host" if polished else None)
    ref = dp.ref_loop(cs, "polished" if polished else "record", None, None, frozenset({"nlt"}))
    soa = lambda a: np.ascontiguousarray(a.reshape(n, -1).T)
    pairs = [("controls", u0), ("states", xs), ("sequences", sq), ("iters", it)]
    pairs += [("status", st), ("rin", ri), ("rout", ro)] if polished else []
    for k, a in pairs:
        assert ref[k].tobytes() == soa(a).tobytes(), k
    assert ref["c"].tobytes() == ref["sequences"][-H * I:].tobytes()
