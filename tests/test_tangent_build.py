"""CPU test of the code objects of the forward-mode kernels (csrc/mpc_tangent.hip, csrc/mpc_rollout_tangent.hip): both
are in the library for gfx950, in both instantiations, and their metadata shows no private segment and no spilled
register -- the per-step quantities live in the handle's workspace, the state tangent in registers."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.mark.skipif(not os.path.exists(READELF), reason="needs llvm-readelf")
def test_tangent_kernels_are_built_for_gfx950_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
            if "tangent_kernel" not in notes:
                continue
            assert "amdgcn-amd-amdhsa--gfx950" in notes
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                if "tangent_kernel" in fields.get(".name", ""):
                    meta[fields[".name"]] = fields
    kinds = sorted((("rollout_" if "rollout_tangent_kernel" in k else "") + ("I2" if "ILi2E" in k else "I1")) for k in meta)
    assert kinds == ["I1", "I2", "rollout_I1", "rollout_I2"], sorted(meta)
    for name, fields in meta.items():
        print(name, {k: fields[k] for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size",
                                            ".vgpr_spill_count", ".sgpr_spill_count")})
        assert int(fields[".private_segment_fixed_size"]) == 0 and int(fields[".vgpr_spill_count"]) == 0, fields
        assert fields[".uses_dynamic_stack"] == "false"
