"""CPU test of the code objects of the compact closed loop (csrc/mpc_compact_loop.hip): the three loop kernels and the
fallback's movers are in the library for gfx950; all three loop kernels have no private segment, no spilled register
and no dynamic stack, and at most 256 VGPRs and AGPRs -- the register kernels (horizon at compile time, H = 4 and 5)
keep the whole step loop in registers, and the step loop of none costs registers beyond one step's (DESIGN.md section
24).  The movers (gather-expand, and the row mover shared with tpc_mpc_rollout_newton) use no private memory either.

Measured on this code: 141 VGPRs at H = 4, 157 at H = 5, 84 for the workspace kernel, 40 for gather-expand."""
import os

import pytest

from tests.model import code_objects as co

LOOP = [("compact_loop_ws_kernel", ())] + [("compact_loop_reg_kernel", (H,)) for H in co.REGISTER_HORIZONS]
MOVERS = [("compact_loop_gather_kernel", ()), ("rollout_newton_move_kernel", (True,))]


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(co.READELF):
        pytest.skip("needs llvm-readelf")
    return co.metadata(r"compact_loop_[a-z_]+_kernel|rollout_newton_move_kernel")


def test_kernels_are_in_the_library(meta):
    assert set(LOOP + MOVERS) <= set(meta), sorted(meta)
    assert not any("compact_exact_" in name for name, _ in LOOP + MOVERS)      # the single solve's build tests select by it


def test_loop_kernels_hold_their_values_in_registers(meta):
    for key in LOOP:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0, (key, f)
        assert int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
        assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, (key, f)


def test_movers_use_no_private_memory(meta):
    for key in MOVERS:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
