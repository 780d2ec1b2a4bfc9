"""CPU test of the code objects of the warm-started exact compact solve (the compact_exact_warm_* kernels of
csrc/mpc_newton_compact.hip, tpc_mpc_solve_batch_compact_exact_from): the six kernels -- register kernels at horizons 4
and 5 and the workspace kernel, each for shared and for per-instance parameters -- are in the library for gfx950; the
register kernels keep their per-step values in registers with the start loaded into them: no private segment, no
spilled VGPR, no dynamic stack, VGPRs + AGPRs at most 256; the workspace kernels have no private segment and no spill
either.  The parents' kernels are still there beside them.  Metadata only."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
REGISTER_HORIZONS = (4, 5)
FAMILIES = ("compact_exact_warm", "compact_exact_warm_rows")
PARENTS = ("compact_exact", "compact_exact_rows")
SHOW = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count",
        ".sgpr_spill_count")


def _metadata():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
            if "compact_exact_" not in notes:
                continue
            assert "amdgcn-amd-amdhsa--gfx950" in notes
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel; the split eats the key
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                fields[".agpr_count"] = re.match(r":\s+(\d+)", block).group(1)
                m = re.search(r"(compact_exact_[a-z_]+_kernel)(?:ILi(\d+)E)?", fields.get(".name", ""))
                if m:
                    meta[(m.group(1), int(m.group(2) or 0))] = fields
    return meta


@pytest.fixture(scope="module")
def meta():
    if not os.path.exists(READELF):
        pytest.skip("needs llvm-readelf")
    return _metadata()


def _kernels(families):
    return ({(f"{fam}_ws_kernel", 0) for fam in families}
            | {(f"{fam}_reg_kernel", H) for fam in families for H in REGISTER_HORIZONS})


def test_the_six_warm_kernels_are_in_the_library(meta):
    assert _kernels(FAMILIES) <= set(meta), sorted(meta)


def test_the_parents_kernels_are_still_there(meta):
    want = _kernels(PARENTS) | {("compact_exact_gather_kernel", 0), ("compact_exact_scatter_kernel", 0)}
    assert want <= set(meta), sorted(meta)


@pytest.mark.parametrize("family", FAMILIES)
def test_register_kernels_hold_the_horizon_and_the_start_in_registers(meta, family):
    for H in REGISTER_HORIZONS:
        f = meta[(f"{family}_reg_kernel", H)]
        print(f"{family} H={H}", {k: f[k] for k in SHOW})
        assert int(f[".private_segment_fixed_size"]) == 0, (H, f)
        assert int(f[".vgpr_spill_count"]) == 0, (H, f)
        assert f[".uses_dynamic_stack"] == "false", (H, f)
        assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, (H, f)


@pytest.mark.parametrize("family", FAMILIES)
def test_workspace_kernels_use_no_private_memory(meta, family):
    f = meta[(f"{family}_ws_kernel", 0)]
    print(family, {k: f[k] for k in SHOW})
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, f
    assert f[".uses_dynamic_stack"] == "false", f
    assert int(f[".vgpr_count"]) + int(f[".agpr_count"]) <= 256, f
