"""GPU test that trajectory_controller_amd.autograd computes what it computed before its two closed-loop Functions, its
two compact expansions and its three copies of the shared-parameter parsing were folded into one each: every public
function reproduces tests/golden/autograd_parent.npz byte for byte, signed zeros included -- outputs, the gradients of
every differentiable input under the recorded cotangents, and the forward_ad tangents where forward mode exists
(tests/model/autograd_parent_common.py has the cases, tests/golden/make_golden_autograd.py made the recording from the
parent's module).  The tests that hold the functions to each other and to the dense checkers would pass if an
operation's order changed within their tolerances; this one would not."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import autograd_parent_common as ap
from trajectory_controller_amd import MpcSolver

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autograd_parent.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def solvers():
    made = {H: MpcSolver(horizon=H, device=0) for H in ap.HORIZONS}
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("case", ap.case_names())
@pytest.mark.parametrize("H", ap.HORIZONS)
def test_same_bytes_as_the_parent(gold, solvers, H, case):
    src = ap.Source(gold=gold)
    got = ap.run_case(H, case, solvers[H], src)
    prefix = f"H{H}/{case}/"
    want = {k for k in gold if k.startswith(prefix) and k not in src.seen}
    assert set(got) == want      # the same outputs, the same inputs reached by a gradient or a tangent
    assert any(k.startswith(prefix + "grad_") for k in want)
    bad = [k for k in sorted(want)
           if not (got[k].shape == gold[k].shape and got[k].dtype == gold[k].dtype and got[k].tobytes() == gold[k].tobytes())]
    assert not bad, bad
