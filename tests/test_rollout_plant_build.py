"""CPU test of the code objects of the plant kernels (csrc/mpc_rollout_newton.hip, mpc_rollout_grad.hip,
mpc_rollout_tangent.hip, mpc_rollout_polish.hip, mpc_rollout.hip): all are in the library for gfx950, each stays in its
parent's occupancy bracket -- the plant's values and tangents are read at the step, not held across the horizon passes --
with no private segment and no spilled register, and the parents' figures are what they were before the plant existed
(DESIGN.md sections 15-17).

Measured on this code: Newton 119 / 90 VGPRs (I = 2 / 1), backward 207 / 172, tangent 160 / 127, fused polish + step
112 / 81, all without private segment or spills."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# kernel name, inputs -> the largest .vgpr_count allowed.  Plant kernels: the brackets of the parents (backward I = 2:
# 256, one wave per SIMD pair as the parent; tangent: 168 / 128, three / four waves per SIMD; Newton: the launch bound).
PLANT_BRACKETS = {("rollout_plant_bwd_kernel", 2): 256, ("rollout_plant_bwd_kernel", 1): 256,
                  ("rollout_plant_fwd_kernel", 2): 168, ("rollout_plant_fwd_kernel", 1): 128,
                  ("rollout_plant_newton_kernel", 2): 128, ("rollout_plant_newton_kernel", 1): 96,
                  ("rollout_plant_polish_step_kernel", 2): 128, ("rollout_plant_polish_step_kernel", 1): 128}
# the parents' recorded figures (172 backward I = 2; 160 / 126 tangent; 118 / 90 Newton, on the polish's
# shared newton_rounds)
PARENT_VGPRS = {("rollout_grad_kernel", 2): 172, ("rollout_tangent_kernel", 2): 160, ("rollout_tangent_kernel", 1): 126,
                ("rollout_newton_kernel", 2): 118, ("rollout_newton_kernel", 1): 90}


def _metadata():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
            if "rollout_" not in notes:
                continue
            assert "amdgcn-amd-amdhsa--gfx950" in notes
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                name = fields.get(".name", "")
                m = re.search(r"(rollout_[a-z_]+_kernel)(?:ILi([12])E)?", name)
                if m:
                    meta[(m.group(1), int(m.group(2) or 0))] = fields
    return meta


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(READELF):
        pytest.skip("needs llvm-readelf")
    return _metadata()


def test_plant_kernels_stay_in_their_parents_brackets(meta):
    assert ("rollout_plant_step_kernel", 0) in meta, sorted(meta)
    for key, cap in PLANT_BRACKETS.items():
        assert key in meta, (key, sorted(meta))
        f = meta[key]
        print(key, {k: f[k] for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count")})
        assert int(f[".vgpr_count"]) <= cap, (key, f[".vgpr_count"])
    for key, f in meta.items():
        if "plant" in key[0]:
            assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, (key, f)
            assert f[".uses_dynamic_stack"] == "false"


def test_parent_kernels_keep_their_figures(meta):
    for key, vgprs in PARENT_VGPRS.items():
        f = meta[key]
        print(key, f[".vgpr_count"])
        assert int(f[".vgpr_count"]) == vgprs, (key, f[".vgpr_count"])
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, (key, f)
