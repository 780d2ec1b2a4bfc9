"""CPU test that the Newton rounds compute what they computed before the polish and the exact compact solve shared one
copy of them (polish::newton_rounds, csrc/mpc_polish_model.h): the host path of a host-only handle reproduces every
array of tests/golden/newton_rounds_parent.npz bit for bit -- tpc_mpc_polish_batch_general with one and two inputs and
tpc_mpc_solve_batch_compact_exact cold, with rows, and warm, at horizons 1, 4, 5, 6, n = 67, with the default round
limit and with one round (scripts/record_newton_rounds.py made the recording from the parent's library).  The tests
that hold the two callers to each other would pass if both changed together; this one would not."""
import os

import numpy as np
import pytest

from tests.model import newton_rounds_common as nr
from trajectory_controller_amd import MpcSolver

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newton_rounds_parent.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_the_recording_contains_what_it_must(gold):
    nr.check_contents(gold)


def check(gold, case, rounds, got, names):
    for k in names:
        want = gold[f"{case}/r{rounds}/{k}"]
        assert nr.same_bits(got[k], want), (case, rounds, k, np.flatnonzero(np.ravel(got[k] != want))[:8])


@pytest.mark.parametrize("H", nr.HS)
@pytest.mark.parametrize("I", nr.INPUTS)
def test_polish_reproduces_the_recorded_bits(gold, I, H):
    case = f"polish_I{I}_H{H}"
    with MpcSolver(horizon=H, device=None) as s:
        for rounds in nr.POLISH_ROUNDS:
            check(gold, case, rounds, nr.run_polish(s, I, H, nr.inputs_of(gold, case), rounds), nr.POLISH_OUT)


@pytest.mark.parametrize("H", nr.HS)
@pytest.mark.parametrize("entry", nr.COMPACT)
def test_compact_solve_reproduces_the_recorded_bits(gold, entry, H):
    case = f"{entry}_H{H}"
    with MpcSolver(horizon=H, device=None) as s:
        for rounds in nr.COMPACT_ROUNDS:
            check(gold, case, rounds, nr.run_compact(s, nr.inputs_of(gold, case), rounds), nr.COMPACT_OUT)
