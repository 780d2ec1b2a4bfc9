"""CPU test of the code objects of the exact compact solve's forward mode (csrc/mpc_compact_tangent.hip): the four
workspace kernels <ROWS, WHOLE> and the four register kernels <4 | 5, ROWS> are in the library for gfx950; none has a
private segment, a spilled register or a dynamic stack; the register kernels (horizon at compile time, row 0 only) keep
their 4 HC per-step values in registers within 256 VGPRs and AGPRs.  Metadata only."""
import itertools
import os

import pytest

from tests.model import code_objects as co

WS = [("compact_tangent_ws_kernel", f) for f in itertools.product((False, True), repeat=2)]      # <ROWS, WHOLE>
REG = [("compact_tangent_reg_kernel", (H, rows)) for H in co.REGISTER_HORIZONS for rows in (False, True)]


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(co.READELF):
        pytest.skip("needs llvm-readelf")
    return co.metadata(r"compact_tangent_[a-z_]+_kernel")


def test_kernels_are_in_the_library(meta):
    assert len(WS) == 4 and len(REG) == 4
    assert set(WS + REG) == set(meta), sorted(meta)


def test_no_kernel_uses_private_memory(meta):
    for key in WS + REG:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".private_segment_fixed_size"]) == 0, (key, f)
        assert int(f[".vgpr_spill_count"]) == 0 and int(f[".sgpr_spill_count"]) == 0, (key, f)
        assert f[".uses_dynamic_stack"] == "false", (key, f)


def test_register_kernels_hold_the_horizon_in_registers(meta):
    for key in REG:
        f = meta[key]
        print(key, co.show(f))
        assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, (key, f)
