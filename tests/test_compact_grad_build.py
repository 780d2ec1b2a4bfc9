"""CPU test of the code objects of the exact compact solve's backward pass (csrc/mpc_compact_grad.hip): the kernels
are in the library for gfx950; the register kernels (horizon at compile time) keep their per-step values in registers
-- no private segment, no spilled register, no dynamic stack, at most 256 VGPRs and AGPRs; the workspace kernel
(run-time H) and the reduce kernel have no private segment and no spill either.  Metadata only."""
import os

import pytest

from tests.model import code_objects as co

SHARED = co.family("compact_grad", False)            # <ROWS> = <false>: [workspace, register H = 4, 5]
REDUCE = ("compact_grad_reduce_kernel", ())


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(co.READELF):
        pytest.skip("needs llvm-readelf")
    return co.metadata(r"compact_grad_[a-z_]+_kernel")


def test_kernels_are_in_the_library(meta):
    assert set(SHARED + [REDUCE]) <= set(meta), sorted(meta)


def test_register_kernels_hold_the_horizon_in_registers(meta):
    for key in SHARED[1:]:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0, (key, f)
        assert int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
        assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, (key, f)


def test_workspace_and_reduce_kernels_use_no_private_memory(meta):
    for key in SHARED[:1] + [REDUCE]:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)
