"""CPU test of the code objects of the warm-started exact compact solve (the WARM instantiations of the kernels of
csrc/mpc_newton_compact.hip, tpc_mpc_solve_batch_compact_exact_from): the six kernels -- register kernels at horizons 4
and 5 and the workspace kernel, each for shared and for per-instance parameters -- are in the library for gfx950; the
register kernels keep their per-step values in registers with the start loaded into them: no private segment, no
spilled VGPR, no dynamic stack, VGPRs + AGPRs at most 256; the workspace kernels have no private segment and no spill
either.  The parents' kernels are still there beside them, kernels of their own: all twelve
instantiations.  Metadata only."""
import os

import pytest

from tests.model import code_objects as co

# <ROWS, WARM>: [workspace, register H = 4, 5]
FAMILIES = {"compact_exact_warm": co.family("compact_exact", False, True),
            "compact_exact_warm_rows": co.family("compact_exact", True, True)}
PARENTS = co.family("compact_exact", False, False) + co.family("compact_exact", True, False)


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(co.READELF):
        pytest.skip("needs llvm-readelf")
    return co.metadata(r"compact_exact_[a-z_]+_kernel")


def test_the_six_warm_kernels_are_in_the_library(meta):
    assert {key for keys in FAMILIES.values() for key in keys} <= set(meta), sorted(meta)


def test_the_parents_kernels_are_still_there(meta):
    want = set(PARENTS) | {("compact_exact_gather_kernel", ()), ("compact_exact_scatter_kernel", ())}
    assert want <= set(meta), sorted(meta)


@pytest.mark.parametrize("family", FAMILIES)
def test_register_kernels_hold_the_horizon_and_the_start_in_registers(meta, family):
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
