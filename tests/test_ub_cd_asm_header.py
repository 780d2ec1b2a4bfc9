"""The hand-written coordinate-descent loop (csrc/mpc_ub_cd_asm.h) is what its generator writes, and keeps the properties its
speed and its safety rest on.  CPU only."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "trajectory_controller_amd", "csrc", "mpc_ub_cd_asm.h")

# every instruction the loop may hold: fp64 arithmetic, selects, LDS reads / writes, scalar control.  No register copy and
# no scalar memory instruction of any kind.
ALLOWED = {"v_fma_f64", "v_mul_f64", "v_add_f64", "v_ldexp_f64", "v_min_f64", "v_max_f64", "v_cmp_lt_f64_e64",
           "v_cmp_neq_f64_e64", "v_cndmask_b32_e64", "v_lshl_add_u32", "v_add_u32_e64", "ds_read2st64_b64", "ds_write_b64",
           "s_waitcnt", "s_nop", "s_cmp_ge_u32", "s_cmp_eq_u64", "s_cbranch_scc1", "s_andn2_b64", "s_and_b64", "s_mov_b64",
           "s_mov_b32", "s_add_u32", "s_branch"}


def _statement(text):
    return [l.strip().strip('"').replace("\\n", "") for l in text.splitlines() if l.strip().startswith('"')
            and l.strip().endswith('\\n"')]


def test_cd_header_is_what_its_generator_writes():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_ub_cd_asm.py")], capture_output=True, text=True,
                         timeout=120)
    assert gen.returncode == 0, gen.stderr[-2000:]
    assert gen.stdout == open(HEADER).read()


def test_cd_loop_instructions_and_alignment():
    lines = _statement(open(HEADER).read())
    top, end = lines.index("TOP%=:"), lines.index("END%=:")
    assert lines[top - 1] == ".p2align 3"
    loop = lines[top + 1:end]
    off = 0
    for l in loop:
        op = l.split()[0]
        assert op in ALLOWED, l
        assert not op.startswith("v_mov")
        if op.startswith("s_"):
            off += 4
        else:
            assert off % 8 == 0, (off, l)   # 8-byte instructions on 8-byte addresses
            off += 8
    # EXEC: saved before the loop, restored before the back edge and on the way out
    assert lines[:top].count("s_mov_b64 %[sexec], exec") == 1
    assert loop[-3:] == ["s_mov_b64 exec, %[sexec]", "s_add_u32 %[sit], %[sit], 1", "s_branch TOP%="]
    assert lines[end + 1] == "s_mov_b64 exec, %[sexec]" and lines[end + 2:] == []
    # the LGKM counter holds 15: never more LDS reads in flight
    n = 0
    for l in loop:
        if l.startswith("ds_"):
            n += 1
            assert n <= 15, l
        m = re.match(r"s_waitcnt lgkmcnt\((\d+)\)", l)
        if m:
            n = min(n, int(m.group(1)))
    src = open(HEADER).read()
    for clob in ('"vcc"', '"scc"', '"exec"', '"memory"'):
        assert clob in src
    # one 1 / Q_diag row per variable in front of x's rows: the offsets the statement uses stay inside the 4H rows
    offs = [int(v) for v in re.findall(r"offset[01]:(\d+)", src)]
    assert max(offs) < 80 and int(re.search(r"ds_write_b64 \S+ \S+ offset:(\d+)", src).group(1)) == 40 * 512
