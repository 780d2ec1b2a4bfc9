"""CPU test of the code objects of the exact compact solve (csrc/mpc_newton_compact.hip): the kernels are in the library
for gfx950; the register kernels (horizon at compile time, H = 4 and 5) keep their per-step values in registers -- no
private segment, no spilled register, no dynamic stack, at most 256 VGPRs and AGPRs; the workspace kernel (run-time H)
and the fallback's gather-expand / scatter kernels have no private segment and no spill either.

Measured on this code: 130 VGPRs at H = 4, 147 at H = 5, 78 for the workspace kernel, 72 / 12 gather / scatter."""
import os

import pytest

from tests.model import code_objects as co

COLD = co.family("compact_exact", False, False)      # <ROWS, WARM> = <false, false>: [workspace, register H = 4, 5]
FALLBACK = [("compact_exact_gather_kernel", ()), ("compact_exact_scatter_kernel", ())]


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(co.READELF):
        pytest.skip("needs llvm-readelf")
    return co.metadata(r"compact_exact_[a-z_]+_kernel")


def test_kernels_are_in_the_library(meta):
    assert set(COLD + FALLBACK) <= set(meta), sorted(meta)


def test_register_kernels_hold_the_horizon_in_registers(meta):
    for key in COLD[1:]:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0, (key, f)
        assert int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
        assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, (key, f)


def test_workspace_and_fallback_kernels_use_no_private_memory(meta):
    for key in COLD[:1] + FALLBACK:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
