"""CPU test of the code objects of the exact compact solve with per-instance parameters (the ROWS instantiations of the
kernels of csrc/mpc_newton_compact.hip and csrc/mpc_compact_grad.hip): the kernels are in the library for gfx950; the
register kernels (horizon at compile time) keep their per-step values in registers -- no private segment, no spilled
register, no dynamic stack, at most 256 VGPRs and AGPRs -- with the ten model values of the lane's instance in VGPRs
beside them; the workspace kernels (run-time H) have no private segment and no spill either.
Metadata only."""
import os

import pytest

from tests.model import code_objects as co

# ROWS = true (the forward's WARM = false): [workspace, register H = 4, 5]
FAMILIES = {"compact_exact_rows": co.family("compact_exact", True, False),
            "compact_grad_rows": co.family("compact_grad", True)}


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(co.READELF):
        pytest.skip("needs llvm-readelf")
    return co.metadata(r"compact_(?:exact|grad)_[a-z]+_kernel")


def test_kernels_are_in_the_library(meta):
    assert {key for keys in FAMILIES.values() for key in keys} <= set(meta), sorted(meta)


@pytest.mark.parametrize("family", FAMILIES)
def test_register_kernels_hold_the_horizon_in_registers(meta, family):
    for key in FAMILIES[family][1:]:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0, (key, f)
        assert int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
        assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, (key, f)


@pytest.mark.parametrize("family", FAMILIES)
def test_workspace_kernels_use_no_private_memory(meta, family):
    key = FAMILIES[family][0]
    f = meta[key]
    print(key, co.show(f))
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, f
    assert f[".uses_dynamic_stack"] == "false", f
    assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, f
