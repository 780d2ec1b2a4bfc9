"""GPU test that the kernels of the Newton rounds compute what they computed before the polish and the exact compact
solve shared one copy of them: a device handle, in DEVICE memory, reproduces every array of
tests/golden/newton_rounds_parent.npz bit for bit, one launch per case (tests/test_newton_rounds_host.py is the same on
the host path and says what the recording holds).  The compact cases at H = 4 and 5 run the register kernels, at H = 1
and 6 the workspace kernels; the polish runs polish_kernel<1> and <2> on arrays wider than the batch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.model import newton_rounds_common as nr
from tests.test_newton_rounds_host import GOLD, check
from trajectory_controller_amd import MpcSolver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("H", nr.HS)
def test_device_reproduces_the_recorded_bits(gold, H):
    with MpcSolver(horizon=H, device=0) as s:
        for I in nr.INPUTS:
            case = f"polish_I{I}_H{H}"
            for rounds in nr.POLISH_ROUNDS:
                check(gold, case, rounds, nr.run_polish(s, I, H, nr.inputs_of(gold, case), rounds, device=True),
                      nr.POLISH_OUT)
        for entry in nr.COMPACT:
            case = f"{entry}_H{H}"
            for rounds in nr.COMPACT_ROUNDS:
                check(gold, case, rounds, nr.run_compact(s, nr.inputs_of(gold, case), rounds, device=True),
                      nr.COMPACT_OUT)
