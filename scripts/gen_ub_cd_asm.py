#!/usr/bin/env python3
"""Generates trajectory_controller_amd/csrc/mpc_ub_cd_asm.h: the fast-build iteration loop of the fp64 LANE_FMA
coordinate-descent kernel (ub_cd_kernel<double, 20, true> of mpc_ub.h, every lane of the wavefront past the screen) as ONE
inline-asm statement with hand-assigned registers.  Everything around the loop -- set-up, the screen, the exact build, the
record, the queue key -- stays compiled C++.

The arithmetic is that of csrc/mpc_ub_model.h operation for operation (the forward pass, the backward sweep, df0 / df1 come
from scripts/ubasm.py, the same emitters as the projected-gradient kernel's); the decisions are those of the compiled fast
build (mpc.h:289-335):
  * the sweep runs i and j DESCENDING and takes |mm| >= |best|: the lowest index among equal maxima wins.  The first
    variable visited always wins its comparison against "none" (|mm| >= 0), so it initialises the running arg-max and
    the second one's select writes the index from two constants: nothing is reset by a register move;
  * stop (mpc.h:310) when |best| < eps, before the update; a lane that stopped keeps sweeping with the others (as in C++)
    but no longer counts iterations or updates;
  * a zero 1 / Q_diag skips the update but the iteration counts (mpc.h:322);
  * x_new = clamp01(fma(-iq, best, x)) (mpc.h:325-326); the iteration number + 1 of a lane's last update is returned, from
    which the caller forms vinit (mpc.h:330-334).

Register / LDS plan (one wavefront per SIMD, as the compiled kernel): x lives in LDS (rows [2H, 4H) of the kernel's
[var][lane] array, 1 / (Q_diag s) in rows [0, 2H)) and is read into v0..v79 at the top of every iteration -- twenty
ds_read2st64_b64, issued ahead of the forward pass that consumes them (at most 15 outstanding: the LGKM counter's
range) -- because exactly one coordinate of a lane changes per iteration and a register array cannot be written at a
per-lane index: the LDS round trip replaces the compiler's select chain.  The forward pass (Z, Y per step) lives in
v80..v159; the winner's x and 1 / Q_diag come back with ONE ds_read2st64_b64 from the two halves of the array.

    python scripts/gen_ub_cd_asm.py [H] > trajectory_controller_amd/csrc/mpc_ub_cd_asm.h
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ubasm

H = int(sys.argv[1]) if len(sys.argv) > 1 else 20
NV = 2 * H
XROW = NV                     # s_cd row of x[0] (rows of 64 doubles = 512 bytes = one st64 unit)
hard = ubasm.hard
X = [hard(2 * q) for q in range(NV)]                       # x[q]
WZ = [hard(2 * NV + 4 * i) for i in range(H)]              # Z[i]
WY = [hard(2 * NV + 4 * i + 2) for i in range(H)]          # Y[i]
_t = 2 * NV + 4 * H
N0, N1, D, GLO, GHI, BM = (hard(_t + 2 * j) for j in range(6))
IDX, ADDR = f"v{_t + 12}", f"v{_t + 13}"
WIN = _t + 14                                               # v[WIN:WIN+3]: the winner's x, then its 1 / Q_diag
BX, IQ = hard(WIN), hard(WIN + 2)
NVGPR = WIN + 4
assert NVGPR <= 256 and NV - 1 <= 64 and 2 * XROW <= 255

C = {n: f"%[{n}]" for n in ("ca", "cc", "cas", "ccs", "cz0", "cq", "cgl0", "cgl1")}
S = {n: f"%[{n}]" for n in ("sgq0", "sgq1", "sgrs0", "sgrs1", "slo1", "seps", "sbig", "s1900")}

FOUR = ("s_",)


def size(l):
    """bytes of one line (labels and directives: 0).  Every vector and LDS instruction here is 8 bytes (VOP3 / DS), every
    scalar one 4 (no literals)"""
    if l.endswith(":") or l.startswith("."):
        return 0
    return 4 if l.startswith(FOUR) else 8


def align(lines):
    """pads with s_nop 0 so that every 8-byte instruction after the loop's .p2align 3 starts on an 8-byte address: an 8-byte
    instruction that straddles costs a lone wavefront 5 cycles instead of 4 (profiles/r05_issue_forms*.txt)"""
    o, off = [], 0
    for l in lines:
        if l.startswith(".p2align"):
            off = 0
        if size(l) == 8 and off % 8:
            o.append("s_nop 0"); off += 4
        o.append(l); off += size(l)
    return o


def mask_and_pick(q, d, x, first, second):
    """mm = max(min(df, g_lo), -g_hi) into BM (first variable) or GLO, and the running arg-max over |mm| (ties: the new one)"""
    mm = BM if first else GLO
    o = [f"v_ldexp_f64 {GLO}, {x}, {S['s1900']}",                  # g_lo: 0 on the bound, else beyond every |df|
         f"v_fma_f64 {GHI}, -{x}, {S['sbig']}, {S['sbig']}",       # g_hi: (1 - x) 2^1000, the same
         f"v_min_f64 {mm}, {d}, {GLO}",
         f"v_max_f64 {mm}, {mm}, -{GHI}"]
    if first:
        return o
    o += [f"v_cmp_lt_f64_e64 vcc, |{GLO}|, |{BM}|",                  # NOT better (no NaN past the screen)
          f"v_cndmask_b32_e64 {BM.lo}, {GLO.lo}, {BM.lo}, vcc",
          f"v_cndmask_b32_e64 {BM.hi}, {GLO.hi}, {BM.hi}, vcc",
          f"v_cndmask_b32_e64 {IDX}, {q}, {q + 1 if second else IDX}, vcc"]
    return o


def gen_loop():
    o = ["s_waitcnt lgkmcnt(0)",                 # (the LGKM counts below assume nothing older in flight)
         "s_mov_b64 %[sexec], exec",
         "s_mov_b32 %[sit], 0",
         ".p2align 3", "TOP%=:",
         "s_cmp_ge_u32 %[sit], %[scd]", "s_cbranch_scc1 END%=",   # it < cd_iters
         "s_cmp_eq_u64 %[slive], 0", "s_cbranch_scc1 END%="]      # some lane has not stopped
    # ---- x of this iteration: pair i = x[2i], x[2i+1] (rows XROW + 2i, + 1)
    issued, waited = [], set()
    def read(i):
        issued.append(i)
        return [f"ds_read2st64_b64 v[{4 * i}:{4 * i + 3}], %[vaddr] offset0:{XROW + 2 * i} offset1:{XROW + 2 * i + 1}"]
    def wait(i):
        if i in waited:
            return []
        after = len(issued) - 1 - issued.index(i)
        waited.update(issued[:issued.index(i) + 1])
        return [f"s_waitcnt lgkmcnt({after})"]
    for i in range(min(15, H)):
        o += read(i)
    # ---- forward pass (Unit::fwd_init / fwd)
    # (one wait per group of steps -- every lone s_waitcnt costs an s_nop as well, to keep the 8-byte instructions aligned --
    #  small groups first, where the data is least likely to be back)
    group_end, g = {}, 0
    for size_ in (2, 2) + (4,) * H:
        if g >= H:
            break
        group_end[g] = min(g + size_, H) - 1
        g += size_
    for i in range(H):
        if i in group_end:
            o += wait(group_end[i])
        zp, yp = (C["cz0"], S["slo1"]) if i == 0 else (WZ[i - 1], WY[i - 1])
        o += ubasm.fwd_step(WZ[i], WY[i], zp, yp, X[2 * i], X[2 * i + 1], C["ca"], C["cas"], C["ccs"])
        if i + 15 < H:
            o += read(i + 15)
    # ---- backward sweep with the arg-max
    for i in range(H - 1, -1, -1):
        if i == H - 1:
            o += ubasm.bwd_last(N0, N1, WZ[i], WY[i], S["sgq0"], S["sgq1"], C["cq"])
        else:
            o += ubasm.bwd_step(N0, N1, WZ[i], WY[i], S["sgq0"], S["sgq1"], C["cq"], C["ca"])
        q = 2 * i + 1
        o += ubasm.df1(D, X[q], N0, N1, S["sgrs1"], C["cgl1"], C["cc"], C["ca"])
        o += mask_and_pick(q, D, X[q], q == NV - 1, q == NV - 2)
        q = 2 * i
        o += ubasm.df0(D, X[q], N1, S["sgrs0"], C["cgl0"], C["cc"])
        o += mask_and_pick(q, D, X[q], q == NV - 1, q == NV - 2)
    # ---- stop test, the winner's update
    o += [f"v_lshl_add_u32 {ADDR}, {IDX}, 9, %[vaddr]",              # &s_cd[best][lane]
          f"ds_read2st64_b64 v[{WIN}:{WIN + 3}], {ADDR} offset0:{XROW} offset1:0",   # x[best], 1 / (Q_diag s)[best]
          f"v_cmp_lt_f64_e64 vcc, |{BM}|, %[seps]",                  # max_df < eps (mpc.h:310-311)
          "s_andn2_b64 %[slive], %[slive], vcc",
          "s_mov_b64 exec, %[slive]",
          f"v_add_u32_e64 %[viter], %[viter], 1",                    # the iteration counts for the lanes still going
          "s_waitcnt lgkmcnt(0)",
          f"v_cmp_neq_f64_e64 vcc, 0, {IQ}",                         # mpc.h:322: a zero Q_diag never updates
          "s_and_b64 exec, %[slive], vcc",
          f"v_fma_f64 {BX}, -{IQ}, {BM}, {BX} clamp",               # project(fma(-iq, best_df, best_x)) (mpc.h:325-326)
          f"v_add_u32_e64 %[vlu], %[sit], 1",                        # (it + 1 of the last update: vinit, mpc.h:330-334)
          f"ds_write_b64 {ADDR}, {BX} offset:{XROW * 512}",
          "s_mov_b64 exec, %[sexec]",
          "s_add_u32 %[sit], %[sit], 1",
          "s_branch TOP%=",
          "END%=:",
          "s_mov_b64 exec, %[sexec]"]
    return align(o)


def loop_instrs(body):
    """instructions of one iteration of the loop (TOP to the back edge), padding included"""
    a, b = body.index("TOP%=:"), body.index("END%=:")
    return sum(1 for l in body[a:b] if size(l))


def gen():
    body = gen_loop()
    n = loop_instrs(body)
    out = []
    out.append(
        "// GENERATED by scripts/gen_ub_cd_asm.py -- do not edit (make -C csrc regen).  The fast-build iteration loop of\n"
        "// ub_cd_kernel<double, %d, true> (mpc_ub.h) as one asm statement with hand-assigned registers; arithmetic: mpc_ub_model.h,\n"
        "// operation for operation; decisions: the compiled fast build's.  %d instructions per iteration (the compiler's: 730).\n"
        "// Register / LDS plan and reasons: scripts/gen_ub_cd_asm.py.\n"
        "//\n"
        "// dlib's mask (mpc.h:298-299) is mm = max(min(df, g_lo), -g_hi) as in the compiled build, with g_lo = ldexp(x, 1900) as\n"
        "// there and g_hi = fma(-x, 2^1000, 2^1000) = (1 - x) 2^1000 (rounded) instead of ldexp(1 - x, 1900): both are +0 exactly\n"
        "// at x = 1 and, for every x < 1 of the unit box, at least 2^-53 2^1000 = 2^947 -- beyond every |df| the screen admits\n"
        "// (ub::fast_stop_ok: |df| <= 3e246 < 2^819) -- so mm, the winner and best_df come out with the same bits.\n"
        "#pragma once\n\nnamespace tpc {\n\n" % (H, n))
    out.append(f"constexpr int kUbCdAsmH = {H}, kUbCdAsmIterInstrs = {n}, kUbCdAsmXRow = {XROW};\n\n")
    out.append(
        "// The uniform model values (g = 1) are asked for in SGPRs (the compiler may hand over VGPRs), the per-lane ones in VGPRs.  vaddr: LDS byte address of\n"
        "// s_cd[0][lane] (rows [0, 2H): 1 / (Q_diag s), rows [2H, 4H): x).  In: live = the lanes that have not stopped, iter, lu = 0.\n"
        "// Out: live, iter (iterations counted per lane), lu (1 + the iteration of the lane's last update, 0 for none).\n"
        "struct UbCdAsmUniform { double gq0, gq1, grs0, grs1, lo1, eps; };\n"
        "#pragma clang diagnostic push\n"
        "#pragma clang diagnostic ignored \"-Winline-asm\"   // (exec is listed on purpose: the statement writes it, and restores it on every path out)\n"
        "TPC_DEV void ub_cd_asm_loop(const UbCdAsmUniform& u, double a, double c, double as1, double cs0, double z0, double q1th,\n"
        "                            double grl0, double grl1, uint32_t vaddr, uint32_t cd_iters, uint64_t& live,\n"
        "                            uint32_t& iter, uint32_t& lu) {\n"
        "    uint64_t sexec;\n"
        "    uint32_t sit;\n"
        "    asm volatile(\n")
    for l in body:
        out.append(f'        "{l}\\n"\n')
    outs = ['[slive] "+s"(live)', '[viter] "+v"(iter)', '[vlu] "+v"(lu)', '[sexec] "=&s"(sexec)', '[sit] "=&s"(sit)']
    ins = ['[sgq0] "s"(u.gq0)', '[sgq1] "s"(u.gq1)', '[sgrs0] "s"(u.grs0)', '[sgrs1] "s"(u.grs1)', '[slo1] "s"(u.lo1)',
           '[seps] "s"(u.eps)', '[sbig] "s"(0x1p1000)', '[s1900] "s"(1900)', '[scd] "s"(cd_iters)',
           '[ca] "v"(a)', '[cc] "v"(c)', '[cas] "v"(as1)', '[ccs] "v"(cs0)', '[cz0] "v"(z0)', '[cq] "v"(q1th)',
           '[cgl0] "v"(grl0)', '[cgl1] "v"(grl1)', '[vaddr] "v"(vaddr)']
    clob = [f'"v{r}"' for r in range(NVGPR)] + ['"vcc"', '"scc"', '"exec"', '"memory"']

    def wrap(items, ind):
        lines, cur = [], ""
        for it in items:
            if len(cur) + len(it) + 2 > 150:
                lines.append(cur.rstrip()); cur = ""
            cur += it + ", "
        lines.append(cur.rstrip().rstrip(","))
        return ("\n" + " " * ind).join(lines)
    out.append("        : " + wrap(outs, 10) + "\n")
    out.append("        : " + wrap(ins, 10) + "\n")
    out.append("        : " + wrap(clob, 10) + ");\n")
    out.append("}\n#pragma clang diagnostic pop\n\n}  // namespace tpc\n")
    return "".join(out)


if __name__ == "__main__":
    sys.stdout.write(gen())
