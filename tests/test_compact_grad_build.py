"""CPU test of the code objects of the exact compact solve's backward pass (csrc/mpc_compact_grad.hip): the kernels
are in the library for gfx950; the register kernels (horizon at compile time) keep their per-step values in registers
-- no private segment, no spilled register, no dynamic stack, at most 256 VGPRs; the workspace kernel (run-time H) and
the reduce kernel have no private segment and no spill either.  Metadata only."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
REGISTER_HORIZONS = (4, 5)
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
            if "compact_grad_" not in notes:
                continue
            assert "amdgcn-amd-amdhsa--gfx950" in notes
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                m = re.search(r"(compact_grad_[a-z_]+_kernel)(?:ILi(\d+)E)?", fields.get(".name", ""))
                if m:
                    meta[(m.group(1), int(m.group(2) or 0))] = fields
    return meta


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(READELF):
        pytest.skip("needs llvm-readelf")
    return _metadata()


def test_kernels_are_in_the_library(meta):
    want = {("compact_grad_ws_kernel", 0), ("compact_grad_reduce_kernel", 0)}
    want |= {("compact_grad_reg_kernel", H) for H in REGISTER_HORIZONS}
    assert want <= set(meta), sorted(meta)


def test_register_kernels_hold_the_horizon_in_registers(meta):
    for H in REGISTER_HORIZONS:
        f = meta[("compact_grad_reg_kernel", H)]
        print(f"H={H}", {k: f[k] for k in SHOW})
        assert int(f[".private_segment_fixed_size"]) == 0, (H, f)
        assert int(f[".vgpr_spill_count"]) == 0, (H, f)
        assert f[".uses_dynamic_stack"] == "false", (H, f)
        assert int(f[".vgpr_count"]) <= 256, (H, f)


def test_workspace_and_reduce_kernels_use_no_private_memory(meta):
    for name in ("compact_grad_ws_kernel", "compact_grad_reduce_kernel"):
        f = meta[(name, 0)]
        print(name, {k: f[k] for k in SHOW})
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, (name, f)
        assert f[".uses_dynamic_stack"] == "false", (name, f)
