"""CPU test of the code objects of the compact closed loop's backward pass (csrc/mpc_compact_loop_grad.hip): the three
kernels are in the library for gfx950; every one of them has no private segment, no spilled VGPR and no dynamic stack,
and at most 256 VGPRs and AGPRs -- the register kernels (horizon at compile time, H = 4 and 5) keep one step's values
in registers and the step loop costs no registers beyond one step's.  The kernels of sections
20 and 24, whose batch reduction this pass shares, are still there.  Metadata only.

Measured on this code: 212 VGPRs at H = 4, 256 at H = 5 (no AGPR), 126 for the workspace kernel."""
import os

import pytest

from tests.model import code_objects as co

GRAD = [("cloop_grad_ws_kernel", ())] + [("cloop_grad_reg_kernel", (H,)) for H in co.REGISTER_HORIZONS]
SECTION_20 = co.family("compact_grad", False) + co.family("compact_grad", True) + [("compact_grad_reduce_kernel", ())]
SECTION_24 = [("compact_loop_ws_kernel", ())] + [("compact_loop_reg_kernel", (H,)) for H in co.REGISTER_HORIZONS]


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(co.READELF):
        pytest.skip("needs llvm-readelf")
    return co.metadata(r"cloop_grad_[a-z_]+_kernel|compact_grad_[a-z_]+_kernel|compact_loop_[a-z_]+_kernel")


def test_kernels_are_in_the_library(meta):
    assert set(GRAD) <= set(meta), sorted(meta)
    assert set(SECTION_20 + SECTION_24) <= set(meta), sorted(meta)
    # the names the other build tests select by
    for name, _ in GRAD:
        assert "compact_exact_" not in name and "compact_grad_" not in name and "compact_loop_" not in name
        assert "tangent_kernel" not in name and not name.startswith("rollout_")
    assert len([k for k in meta if k[0].startswith("cloop_grad_")]) == len(GRAD)


def test_every_kernel_holds_its_values_in_registers(meta):
    for key in GRAD:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0, (key, f)
        assert int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
        assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, (key, f)


def test_shared_reduction_kernels_are_as_before(meta):
    """block_partials moved into a header and the reduce launch is shared: section 20's kernels keep their shape"""
    for key in SECTION_20:
        f = meta[key]
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
    assert int(meta[("compact_grad_reg_kernel", (5, False))][".vgpr_count"]) == 212
    assert int(meta[("compact_grad_reg_kernel", (4, False))][".vgpr_count"]) == 162
