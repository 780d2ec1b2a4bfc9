"""tests/model/code_objects.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The code-object metadata of the built library's gfx950 kernels, for the CPU tests that hold kernels to "no private
segment, no spill" (tests/test_compact_*_build.py): one reader, keyed by kernel name and template arguments.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
REGISTER_HORIZONS = (4, 5)      # the horizons the compact entries compile in (compact_*_reg_kernel<HC, ..>)
SHOW = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count",
        ".sgpr_spill_count", ".group_segment_fixed_size")


def metadata(name_regex, lib=None):
    """{(kernel name, template arguments): fields} of the library's kernels whose name matches name_regex; the template
    arguments as a tuple of ints and bools, () for a kernel that is no template -- compact_exact_reg_kernel<4, false,
    true> is ("compact_exact_reg_kernel", (4, False, True)).  lib: another build of the library to read"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = lib or os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
            if not re.search(name_regex, notes):
                continue
            assert "amdgcn-amd-amdhsa--gfx950" in notes
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel; the split eats the key
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                fields[".agpr_count"] = re.match(r":\s+(\d+)", block).group(1)
                m = re.search(rf"({name_regex})(?:I((?:L[ib]\d+E)+)E)?", fields.get(".name", ""))
                if m:
                    args = tuple(int(x) if kind == "i" else x == "1"
                                 for kind, x in re.findall(r"L([ib])(\d+)E", m.group(2) or ""))
                    meta[(m.group(1), args)] = fields
    return meta


def family(entry, *flags):
    """the keys of the three instantiations a compact entry launches for one choice of its boolean template arguments:
    the workspace kernel and the register kernel at both horizons"""
    return [(f"{entry}_ws_kernel", flags)] + [(f"{entry}_reg_kernel", (H,) + flags) for H in REGISTER_HORIZONS]


def show(fields):
    return {k: fields[k] for k in SHOW}
