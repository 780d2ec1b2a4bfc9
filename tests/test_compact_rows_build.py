"""CPU test of the code objects of the exact compact solve with per-instance parameters (the compact_exact_rows_* kernels
of csrc/mpc_newton_compact.hip and the compact_grad_rows_* kernels of csrc/mpc_compact_grad.hip): the kernels are in the
library for gfx950; the register kernels (horizon at compile time) keep their per-step values in registers -- no private
segment, no spilled register, no dynamic stack, at most 256 VGPRs -- with the ten model values of the lane's instance in
VGPRs beside them; the workspace kernels (run-time H) have no private segment and no spill either (DESIGN.md section
21).  Metadata only."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
REGISTER_HORIZONS = (4, 5)
FAMILIES = ("compact_exact_rows", "compact_grad_rows")
SHOW = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size")


def _metadata():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
            if "_rows_" not in notes:
                continue
            assert "amdgcn-amd-amdhsa--gfx950" in notes
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                m = re.search(r"(compact_(?:exact|grad)_rows_[a-z]+_kernel)(?:ILi(\d+)E)?", fields.get(".name", ""))
                if m:
                    meta[(m.group(1), int(m.group(2) or 0))] = fields
    return meta


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(READELF):
        pytest.skip("needs llvm-readelf")
    return _metadata()


def test_kernels_are_in_the_library(meta):
    want = {(f"{fam}_ws_kernel", 0) for fam in FAMILIES}
    want |= {(f"{fam}_reg_kernel", H) for fam in FAMILIES for H in REGISTER_HORIZONS}
    assert want <= set(meta), sorted(meta)


@pytest.mark.parametrize("family", FAMILIES)
def test_register_kernels_hold_the_horizon_in_registers(meta, family):
    for H in REGISTER_HORIZONS:
        f = meta[(f"{family}_reg_kernel", H)]
        print(f"{family} H={H}", {k: f[k] for k in SHOW})
        assert int(f[".private_segment_fixed_size"]) == 0, (H, f)
        assert int(f[".vgpr_spill_count"]) == 0, (H, f)
        assert f[".uses_dynamic_stack"] == "false", (H, f)
        assert int(f[".vgpr_count"]) <= 256, (H, f)


@pytest.mark.parametrize("family", FAMILIES)
def test_workspace_kernels_use_no_private_memory(meta, family):
    f = meta[(f"{family}_ws_kernel", 0)]
    print(family, {k: f[k] for k in SHOW})
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, f
    assert f[".uses_dynamic_stack"] == "false", f
    assert int(f[".vgpr_count"]) <= 256, f
