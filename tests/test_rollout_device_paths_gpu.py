"""GPU tests of the device side of the closed-loop entries and their derivatives: tpc_mpc_rollout, _record, _polished,
_newton, _plant, the two backwards and the three forwards, called through the C entries on a device handle in HOST
(staged) and DEVICE memory with SOME of their optional arrays.  What is under test is layout, not arithmetic: the
working set's leading dimension, the staging offsets that depend on which arrays were given, the fallback's compact
batch with its gather and scatter, the memsets for a missing controller state, stale layouts on one handle, and the
stream the work is queued on.

Every comparison is byte equality with a reference that no device call produced (tests/model/rollout_device_paths.py:
the host-only handle where it serves the entry, the oracle's loop with the host-only polish for the solve-based loops,
"the polished loop where FALLBACK_NONE says first_unverified < steps" for FALLBACK_SOLVE).  The device handle runs the
LANE family, which is the oracle's bits.  Every array is wider than the batch (ld = n + 13, the batch at column 5,
ld_d = n + 29 for the disturbance; ld_d = 0, the io's ld, exists for ddisturbance / tdisturbance only: the loops refuse
a disturbance with ld_d < n), outputs are filled with a sentinel and their padding must keep it, an output that is not
given is not allocated, and one more sentinel-filled array of the largest output's size lives beside each call's
arrays and must stay untouched.  tests/test_rollout_device_paths_host.py asserts what the inputs have to be (the
fallback sets' sizes); first_unverified is compared with the host's here, so the fallback set is the predicted one."""
import pytest

torch = pytest.importorskip("torch")

from tests.model import rollout_device_paths as dp
from trajectory_controller_amd import MpcSolver, capi

pytestmark = pytest.mark.gpu
MEM = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
# (loop, mode, fallback): the parent entries, then tpc_mpc_rollout_plant with the plant's arrays, a disturbance, both
VARIANTS = [("rollout", None, None), ("record", None, None), ("polished", None, None), ("newton", None, "none"),
            ("newton", None, "solve")]
VARIANTS += [(kind, mode, fb) for mode in dp.MODES[1:]
             for kind, fb in (("record", None), ("polished", None), ("newton", "none"), ("newton", "solve"))]
LOOP_CASES = [(shape, v) for shape in dp.SHAPES for v in VARIANTS]
# the batch whose fallback set is one instance: ldc = 64 with one live lane; the disturbance's rows last in the batch
LOOP_CASES += [("one", v) for v in VARIANTS if v[2] == "solve"]


def _case(shape):
    return dp.one_fallback_case() if shape == "one" else dp.case(*shape)


def _solver(cs):
    return MpcSolver(horizon=cs.H, device=0, algo="lane")


# ---- 1, 2. optional arrays of the loops; the fallback's compact batch ---------------------------------------------------

@MEM
@pytest.mark.parametrize("shape,variant", LOOP_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else v)
def test_loop_with_subsets_of_its_optional_arrays(shape, variant, device):
    kind, mode, fallback = variant
    cs, lib = _case(shape), capi.load_library()
    with _solver(cs) as s:
        for present in dp.subsets(kind, mode):
            res = dp.run_loop(lib, s, cs, dp.wide(cs.n, device), kind, mode, fallback, present)
            try:
                dp.check_loop(cs, kind, mode, fallback, present, *res)
            except AssertionError as e:
                raise AssertionError(f"given {sorted(present)}: {e}") from e


# ---- 3. optional inputs and outputs of the derivative entries -----------------------------------------------------------

def _backward_calls(mode):
    """(outputs, inputs, ld_d = 0) of every backward call"""
    outs = dp.grad_outputs(mode)
    calls = [(outs, {}, False)] + [((k,), {}, False) for k in outs] + [(tuple(o for o in outs if o != k), {}, False)
                                                                      for k in outs]
    calls += [(outs, dict(gx=False), False), (outs, dict(gu=False), False)]
    calls += [(dp.grad_outputs(mode, nlt=False), dict(nlt=False), False)]
    if mode is not None:
        calls += [(("ddisturbance",), {}, True), (outs, {}, True)]
    return calls


@MEM
@pytest.mark.parametrize("mode", dp.MODES, ids=str)
@pytest.mark.parametrize("shape", dp.SHAPES, ids=str)
def test_backward_with_subsets_of_its_outputs_and_inputs(shape, mode, device):
    cs, lib = _case(shape), capi.load_library()
    with _solver(cs) as s:
        for outs, inputs, zero in _backward_calls(mode):
            res = dp.run_backward(lib, s, cs, dp.wide(cs.n, device), mode, outs, ld_d_zero=zero, **inputs)
            try:
                dp.check_backward(cs, mode, *res, **inputs)
            except AssertionError as e:
                raise AssertionError(f"outputs {outs}, {inputs}, ld_d = 0: {zero}: {e}") from e


@MEM
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("mode", dp.MODES + ("single",), ids=str)
@pytest.mark.parametrize("shape", dp.SHAPES, ids=str)
def test_forward_with_each_tangent_alone(shape, mode, K, device):
    cs, lib = _case(shape), capi.load_library()
    single = mode == "single"
    mode = None if single else mode
    names = dp.tangent_names(mode, single)
    calls = [((k,), True, False) for k in names] + [(names, True, False), ((), True, False)]
    if not single:
        calls += [(names, False, False), (("Q",), False, False)]        # tstates is optional
    if mode is not None:
        calls += [(("disturbance",), True, True), (names, True, True)]   # ld_d = 0: tdisturbance has the io's ld
    with _solver(cs) as s:
        for given, want_states, zero in calls:
            res = dp.run_forward(lib, s, cs, dp.wide(cs.n, device), mode, K, given, want_states, single, zero)
            try:
                dp.check_forward(cs, mode, K, given, single, *res)
            except AssertionError as e:
                raise AssertionError(f"tangents {given}, tstates {want_states}, ld_d = 0: {zero}: {e}") from e


# ---- 4. stale layouts: a large call, a small one with the fewest arrays, the large one again, on one handle -------------

@pytest.mark.parametrize("entry", ["newton_solve", "backward", "forward"])
def test_layouts_of_an_earlier_call_do_not_leak_into_the_next(entry):
    big, small, lib = dp.case(2, 10, 4, 130), dp.case(2, 10, 4, 65), capi.load_library()
    everything = frozenset(dp.LOOP_OPTIONAL["newton"])
    with _solver(big) as s:
        for device in (False, True):     # HOST memory first: the staging buffer keeps the large call's size
            for cs, full in ((big, True), (small, False), (big, True)):
                mem = dp.wide(cs.n, device)
                if entry == "newton_solve":
                    present = everything if full else frozenset()
                    dp.check_loop(cs, "newton", "both", "solve", present,
                                  *dp.run_loop(lib, s, cs, mem, "newton", "both", "solve", present))
                elif entry == "backward":
                    outs = dp.grad_outputs("both") if full else ("dC",)
                    inputs = {} if full else dict(gu=False, nlt=False)
                    dp.check_backward(cs, "both", *dp.run_backward(lib, s, cs, mem, "both", outs, **inputs), **inputs)
                else:
                    names, K = (dp.tangent_names("both"), 3) if full else (("R",), 1)
                    dp.check_forward(cs, "both", K, names, False,
                                     *dp.run_forward(lib, s, cs, mem, "both", K, names, want_states=full))


# ---- 5. a side stream ---------------------------------------------------------------------------------------------------

def test_chains_on_a_side_stream():
    """Everything on one non-blocking stream, DEVICE memory: busywork, then the copies from pinned memory into arrays
    that hold NaN, then the entries with that stream; only that stream is waited for.  A step of an entry that went to
    the null stream would read the NaNs (or find the outputs' sentinels overwritten later).  No flags are asked for, so
    no entry waits by itself except for the fallback's count."""
    cs, lib = dp.case(2, 10, 4, 130), capi.load_library()
    stream = torch.cuda.Stream()
    with _solver(cs) as s:
        mem = dp.wide(cs.n, True, stream)
        everything = frozenset(dp.LOOP_OPTIONAL["newton"])
        outs, names = dp.grad_outputs("both"), dp.tangent_names("both")
        loop = dp.run_loop(lib, s, cs, mem, "newton", "both", "solve", everything, launch_only=True)
        back = dp.run_backward(lib, s, cs, mem, "both", outs, launch_only=True)
        fwd = dp.run_forward(lib, s, cs, mem, "both", 3, names, launch_only=True)
        stream.synchronize()
        dp.check_loop(cs, "newton", "both", "solve", everything, *loop)
        dp.check_backward(cs, "both", *back)
        dp.check_forward(cs, "both", 3, names, False, *fwd)

        mem = dp.wide(cs.n, True, stream)
        pol = dp.run_polish(lib, s, cs, mem, launch_only=True)
        everything = frozenset(dp.LOOP_OPTIONAL["polished"])
        loop = dp.run_loop(lib, s, cs, mem, "polished", None, None, everything, launch_only=True)
        stream.synchronize()
        dp.check_polish(cs, *pol)
        dp.check_loop(cs, "polished", None, None, everything, *loop)
