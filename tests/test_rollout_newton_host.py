"""CPU tests of the Newton-first closed loop (tpc_mpc_rollout_newton, MpcSolver.rollout_newton) on a host-only handle,
TPC_MPC_NEWTON_FALLBACK_NONE, tol 1e-9, 8 rounds: the loop against its definition composed from the public polish
entry, every verified loop against the dense closed loop and the oracle-based polished replay, how much of a batch the
Newton rounds carry, the entry's argument checks and edge cases, and the code object of the new kernels."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.model import mpc_rollout_polish_ref as rp
from tests.test_rollout_polish_host import BOUND as POLISHED_BOUND
from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd.synth import general_inputs

NAMES = rd.NAMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, ROUNDS = 1e-9, 8
SHAPES = [(1, 4, 8), (2, 10, 10), (2, 20, 6), (1, 20, 6)]     # (I, H, S)
N = 40
COVERAGE_CAP = 0.10     # on synth.general_inputs seed 5 at most 10 % of the instances may leave the Newton pass

# Optimality of the instances the Newton pass carries through every step, measured on the CPU (host-only handle):
# the largest deviation of u0 / states from the dense closed loop on the loop's own active sets, per input kind over
# the four shapes with new_last_targets:
#   synth.general_inputs seed 5, n = 40      1.0e-15, 2.7e-14, 3.06e-13, 1.3e-13   (carried 40, 38, 38, 40 of 40)
#   mpc_rollout_dense.batch,     n = 40      3.6e-15, 5.0e-14, 1.6e-13, 2.6e-13    (carried 38, 22, 18, 22 of 40)
# The bound is 10x the largest, the convention of tests/test_rollout_polish_host.py.  Against the oracle-based
# polished replay the same instances differ by at most 2.0e-14 (asserted: this bound plus that loop's, 2.2e-11).
MEASURED = 3.06e-13
BOUND = 10 * MEASURED


def inputs(kind, I, H, S, n=N, with_nlt=True):
    """(th AoS dict, nlt [n, S, 2] | None)"""
    if kind == "batch":
        return rd.batch(I, H, S, n, seed=H + I, with_nlt=with_nlt)
    g = general_inputs(H, n, I=I, seed=5)
    th = {k: g[k] for k in NAMES}
    nlt = None
    if with_nlt:
        nlt = th["targets"][:, -1:, :] + 0.05 * np.random.default_rng(11).standard_normal((n, S, 2))
    return th, nlt


def soa_inputs(th, nlt, n):
    return [dense.soa(th[k], n) for k in NAMES], (None if nlt is None else dense.soa(nlt, n))


def newton_host(I, H, S, ins, nlt, tol=TOL, rounds=ROUNDS, controls=None, v=None):
    """MpcSolver.rollout_newton on a host-only handle; (controls, states, sequences, status, iters, first, res_in,
    res_out, flags)"""
    n = ins[0].shape[1]
    ri, ro = np.full((S, n), 7.0), np.full((S, n), 7.0)
    with MpcSolver(horizon=H, device=None) as s:
        u, x, q, st, it, first = s.rollout_newton(S, *ins, nlt, controls=controls, v_state=v, inputs=I, tol=tol,
                                                  max_rounds=rounds, fallback="none", want_iters=True,
                                                  residuals=(ri, ro))
        return u, x, q, st, it, first, ri, ro, s.last_flags


def composed(I, H, S, ins, nlt, tol=TOL, rounds=ROUNDS):
    """The definition, step by step: dlib's shift of the carried controls, polish_batch_general on a host-only handle,
    the plant update of mpc_rollout_polish_ref.replay operation for operation, the target shift and set_last_target.
    An instance is dropped at its first unverified step; its rows from there on are status -1 and zeros."""
    n = ins[0].shape[1]
    model, A, B, Cc = ins[:7], ins[0], ins[1], ins[2]
    x, T, c = ins[7].copy(), ins[8].copy(), np.zeros((H * I, n))
    alive, first = np.ones(n, dtype=bool), np.full(n, S, dtype=np.int32)
    u, xs, sq = np.zeros((S * I, n)), np.zeros((S * 2, n)), np.zeros((S * H * I, n))
    st, ri, ro = np.full((S, n), -1, dtype=np.int32), np.zeros((S, n)), np.zeros((S, n))
    with MpcSolver(horizon=H, device=None) as s, np.errstate(all="ignore"):
        for k in range(S):
            c[:-I] = c[I:].copy()                  # mpc.h:231-232
            _, st_k, ri_k, ro_k = s.polish_batch_general(*model, x, T, c, tol=tol, max_rounds=rounds, inputs=I)
            ok = alive & (st_k >= 0)
            first[alive & ~ok] = k
            alive = ok
            u0 = c[:I]
            xn = np.empty((2, n))
            for r in range(2):
                bu = B[r * I] * u0[0]
                if I == 2:
                    bu = bu + B[r * I + 1] * u0[1]
                xn[r] = ((A[2 * r] * x[0] + A[2 * r + 1] * x[1]) + bu) + Cc[r]
            x = xn
            u[k * I:(k + 1) * I, ok], xs[2 * k:2 * k + 2, ok] = u0[:, ok], x[:, ok]
            sq[k * H * I:(k + 1) * H * I, ok] = c[:, ok]
            st[k, ok], ri[k, ok], ro[k, ok] = st_k[ok], ri_k[ok], ro_k[ok]
            T[:-2] = T[2:].copy()
            if nlt is not None and k + 1 < S:
                T[-2:] = nlt[2 * (k + 1):2 * (k + 1) + 2]
    c[:, ~alive] = 0.0
    return u, xs, sq, st, first, ri, ro, c


def composed_from(I, H, ins, start, tol=TOL, rounds=ROUNDS):
    """one step of the definition from a carried sequence: (sequence row or zeros, status row)"""
    c = start.copy()
    c[:-I] = c[I:].copy()
    with MpcSolver(horizon=H, device=None) as s:
        _, st, _, _ = s.polish_batch_general(*ins[:9], c, tol=tol, max_rounds=rounds, inputs=I)
    c[:, st < 0] = 0.0
    return c, st.reshape(1, -1)


@functools.lru_cache(maxsize=None)
def newton_case(kind, I, H, S, with_nlt):
    th, nlt = inputs(kind, I, H, S, with_nlt=with_nlt)
    ins, nl = soa_inputs(th, nlt, N)
    return th, nlt, ins, nl, newton_host(I, H, S, ins, nl)


def aos(a, n, S, rest):
    return np.ascontiguousarray(a.T).reshape((n, S) + rest)


def test_symbol_header_and_abi_version():
    lib = capi.load_library()
    assert "tpc_mpc_rollout_newton" in capi.EXPORTS and hasattr(lib, "tpc_mpc_rollout_newton")
    assert lib.tpc_mpc_abi_version() == 5 == capi.ABI_VERSION
    with open(os.path.join(ROOT, "include", "tpc_mpc.h")) as f:
        text = f.read()
    assert "int tpc_mpc_rollout_newton(" in text
    assert "#define TPC_MPC_NEWTON_FALLBACK_SOLVE 0" in text and "#define TPC_MPC_NEWTON_FALLBACK_NONE 1" in text
    assert (capi.NEWTON_FALLBACK_SOLVE, capi.NEWTON_FALLBACK_NONE) == (0, 1)


# ---- 1. the reference loop -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_nlt", [True, False], ids=["nlt", "nonlt"])
@pytest.mark.parametrize("I,H,S", SHAPES)
@pytest.mark.parametrize("kind", ["general", "batch"])
def test_loop_is_its_definition_bit_for_bit(kind, I, H, S, with_nlt):
    """Every row of every instance: up to first_unverified the composed loop's bits, from there on status -1 and
    zeros.  Nothing is left out of the comparison."""
    _, _, ins, nl, (u, x, q, st, it, first, ri, ro, flags) = newton_case(kind, I, H, S, with_nlt)
    wu, wx, wq, wst, wfirst, wri, wro, wc = composed(I, H, S, ins, nl)
    print(f"{kind} I={I} H={H} S={S}: first_unverified < S for {int((wfirst < S).sum())}/{N}, rounds "
          f"{wst[wst >= 0].mean() if (wst >= 0).any() else float('nan'):.2f} mean, {int(wst.max())} max")
    assert first.dtype == np.int32 and np.array_equal(first, wfirst)
    for name, a, b in (("controls", u, wu), ("states", x, wx), ("sequences", q, wq), ("status", st, wst),
                       ("residual_in", ri, wri), ("residual_out", ro, wro)):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert a.tobytes() == b.tobytes(), name
    assert not it.any()
    # rows from first_unverified on, as defined
    for i in np.flatnonzero(first < S):
        k = first[i]
        assert np.all(st[k:, i] == -1) and not ri[k:, i].any() and not ro[k:, i].any()
        assert not u[k * I:, i].any() and not x[2 * k:, i].any() and not q[k * H * I:, i].any()
        assert np.all(st[:k, i] >= 0) and np.all(ro[:k, i] <= TOL)
    assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((first < S).any())
    assert flags & ~capi.FLAG_NOT_POLISHED == 0


def test_controller_state_out():
    """controls_inout = the last step's sequence, v_inout = the same (what dlib resets v to); a carried-in sequence is
    shifted at step 0 as tpc_mpc_rollout does it."""
    I, H, S = 2, 10, 5
    th, nlt = inputs("batch", I, H, S)
    ins, nl = soa_inputs(th, nlt, N)
    c, v = np.zeros((H * I, N)), np.full((H * I, N), 3.0)
    u, x, q, st, it, first, *_ = newton_host(I, H, S, ins, nl, controls=c, v=v)
    assert c.tobytes() == q[(S - 1) * H * I:].tobytes() and v.tobytes() == c.tobytes()
    assert (first < S).any() and not c[:, first < S].any() and c[:, first == S].any()
    # a start that is not zero: the shift is applied at step 0 too
    start = np.concatenate([np.zeros((I, N)), q[:(H - 1) * I]])
    u2, _, q2, st2, _, first2, *_ = newton_host(I, H, 1, ins, None, controls=start.copy())
    w = composed_from(I, H, ins, start)
    assert q2.tobytes() == w[0].tobytes() and st2.tobytes() == w[1].tobytes()


# ---- 2. optimality ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("I,H,S", SHAPES)
@pytest.mark.parametrize("kind", ["general", "batch"])
def test_carried_instances_are_the_dense_closed_loop(kind, I, H, S):
    th, nlt, _, _, (u, x, q, st, _, first, *_) = newton_case(kind, I, H, S, True)
    whole = first == S
    dev = rp.deviation_from_optimum(I, H, S, th, nlt, aos(u, N, S, (I,)), aos(x, N, S, (2,)), aos(q, N, S, (H, I)))
    print(f"{kind} I={I} H={H} S={S}: carried {int(whole.sum())}/{N}, largest deviation {dev[whole].max():.3e} "
          f"(bound {BOUND:.3e})")
    assert whole.any()
    assert dev[whole].max() <= BOUND, dev[whole].max()


@pytest.mark.parametrize("I,H,S", SHAPES)
@pytest.mark.parametrize("kind", ["general", "batch"])
def test_carried_instances_agree_with_the_polished_replay(kind, I, H, S):
    """The oracle-based polished loop (first-order solve, then the polish) on the same inputs: both loops return every
    step's verified optimum, each within its own asserted deviation of it, so they agree to the sum of the two."""
    th, nlt, _, _, (u, x, q, st, _, first, *_) = newton_case(kind, I, H, S, True)
    ru, rx, rq, rst, *_ = rp.replay(I, H, S, th, nlt, tol=TOL, max_rounds=ROUNDS, polisher="host")
    both = (first == S) & (rst >= 0).all(axis=1)
    du = np.abs(aos(u, N, S, (I,)) - ru)[both].max()
    dx = np.abs(aos(x, N, S, (2,)) - rx)[both].max()
    print(f"{kind} I={I} H={H} S={S}: compared {int(both.sum())}/{N}, |du0| {du:.3e} |dx| {dx:.3e} "
          f"(bound {BOUND + POLISHED_BOUND:.3e})")
    assert both.sum() >= 0.5 * (first == S).sum() and both.any()
    assert max(du, dx) <= BOUND + POLISHED_BOUND


# ---- 3. coverage -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("I,H,S,n", [(2, 20, 6, 200), (1, 20, 6, 200), (2, 40, 5, 60), (2, 10, 10, 200)])
def test_newton_pass_carries_the_reference_kind_of_problem(I, H, S, n):
    th, nlt = inputs("general", I, H, S, n=n)
    ins, nl = soa_inputs(th, nlt, n)
    *_, st, _, first, _, _, _ = newton_host(I, H, S, ins, nl)
    share = float((first < S).mean())
    hist = np.bincount(first, minlength=S + 1)
    print(f"general_inputs seed 5 I={I} H={H} S={S}: unverified {int((first < S).sum())}/{n}, first_unverified "
          f"histogram {hist.tolist()}, mean rounds per step {[round(float(st[k][st[k] >= 0].mean()), 2) for k in range(S)]}")
    assert share <= COVERAGE_CAP, share


@pytest.mark.parametrize("I,H,S", SHAPES)
def test_adversarial_batch_has_both_kinds(I, H, S):
    *_, (u, x, q, st, _, first, *_) = newton_case("batch", I, H, S, True)
    print(f"mpc_rollout_dense.batch I={I} H={H} S={S}: unverified {int((first < S).sum())}/{N}")
    assert (first < S).any() and (first == S).any()


# ---- 4. ABI ----------------------------------------------------------------------------------------------------------

@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


def _raw(h, H, I, S, n, tol=1e-9, rounds=8, dtype=capi.F64, mem=capi.HOST, q=True, ld=None, fallback=1, flags0=99):
    th, _ = rd.batch(I if I in (1, 2) else 2, 4, 3, 3, seed=0)
    ins = {k: dense.soa(th[k], 3) for k in NAMES}
    p = capi.default_params(20, dtype=dtype)
    p.horizon = H
    ptr = lambda a: a.ctypes.data
    io = capi.GeneralIO(inputs=I, n=n, ld=n if ld is None else ld, A=ptr(ins["A"]), B=ptr(ins["B"]), C=ptr(ins["C"]),
                        Q=ptr(ins["Q"]), R=ptr(ins["R"]), lower=ptr(ins["lo"]), upper=ptr(ins["hi"]), x0=ptr(ins["x0"]),
                        targets=ptr(ins["targets"]))
    qq = capi.Polish(tol=tol, max_rounds=rounds)
    cu, cx = np.full((max(S, 1) * I, 3), 7.0), np.full((max(S, 1) * 2, 3), 7.0)
    first = np.full(3, -5, dtype=np.int32)
    flags = C.c_uint32(flags0)
    rc = capi.load_library().tpc_mpc_rollout_newton(h, C.byref(p), C.byref(io), S, None, C.byref(qq) if q else None,
                                                    fallback, ptr(cu), ptr(cx), None, None, ptr(first),
                                                    C.byref(flags), mem, None)
    return rc, flags.value, cu, cx, first


def test_argument_errors(host_handle):
    lib = capi.load_library()
    I, H, S, n = 2, 4, 3, 3
    msg = lambda: lib.tpc_mpc_last_error(host_handle)

    def bad(**kw):
        args = dict(H=H, I=I, S=S, n=n)
        args.update(kw)
        rc, _, cu, cx, first = _raw(host_handle, **args)
        assert np.all(cu == 7.0) and np.all(cx == 7.0) and np.all(first == -5)     # nothing is written on an error
        return rc
    assert bad(q=False) == 1 and b"polish" in msg()
    for kw in (dict(tol=0.0), dict(tol=-1e-9), dict(tol=np.nan), dict(rounds=-1)):
        assert bad(**kw) == 1 and b"tol > 0" in msg(), kw
    for fb in (2, -1, 7):
        assert bad(fallback=fb) == 1 and b"fallback" in msg()
    assert bad(dtype=capi.F32) == 1 and b"fp64" in msg()
    assert bad(S=-1) == 1 and b"steps" in msg()
    assert bad(H=65) == 4 and bad(H=0) == 4
    assert bad(I=3) == 1
    assert bad(ld=n - 1) == 1
    # the fallback solve needs the device, and so does DEVICE memory; the argument checks come first
    assert bad(fallback=0) == 6 and b"host-only" in msg()
    assert bad(fallback=0, tol=0.0) == 1
    assert bad(mem=capi.DEVICE) == 6
    p = capi.default_params(4)
    assert lib.tpc_mpc_rollout_newton(None, C.byref(p), None, S, None, None, 1, None, None, None, None, None, None,
                                      capi.HOST, None) == 1


def test_empty_calls(host_handle):
    for kw in (dict(n=0), dict(S=0)):
        args = dict(H=4, I=2, S=3, n=3)
        args.update(kw)
        for fb in (0, 1):     # FALLBACK_SOLVE has no host path at all: NO_DEVICE, whatever the sizes
            rc, flags, cu, cx, first = _raw(host_handle, fallback=fb, **args)
            assert np.all(cu == 7.0) and np.all(cx == 7.0) and np.all(first == -5)
            assert (rc, flags) == ((0, 0) if fb == 1 else (6, 99))
    rc, flags, cu, cx, first = _raw(host_handle, H=4, I=2, S=3, n=3)
    assert rc == 0 and not np.any(cu == 7.0) and np.all((first >= 0) & (first <= 3))


@pytest.mark.parametrize("what,flag", [("nan", capi.FLAG_NONFINITE), ("R", capi.FLAG_BAD_MODEL),
                                       ("bounds", capi.FLAG_BAD_MODEL)])
def test_invalid_instance_among_good_ones(what, flag):
    I, H, S, bad = 2, 10, 5, 17
    th, nlt = inputs("general", I, H, S)
    ins, nl = soa_inputs(th, nlt, N)
    clean = newton_host(I, H, S, ins, nl)
    ins = [a.copy() for a in ins]
    if what == "nan":
        ins[7][1, bad] = np.nan
    elif what == "R":
        ins[4][1, bad] = 0.0
    else:
        ins[6][0, bad] = ins[5][0, bad] - 0.1
    u, x, q, st, it, first, ri, ro, flags = newton_host(I, H, S, ins, nl)
    others = np.arange(N) != bad
    assert first[bad] == 0 and np.all(st[:, bad] == -1) and not ri[:, bad].any() and not ro[:, bad].any()
    assert not u[:, bad].any() and not x[:, bad].any() and not q[:, bad].any()
    for a, b in zip((u, x, q, st, first, ri, ro), (clean[0], clean[1], clean[2], clean[3], clean[5], clean[6], clean[7])):
        assert np.ascontiguousarray(a[..., others]).tobytes() == np.ascontiguousarray(b[..., others]).tobytes()
    # its own flag, and NOT_POLISHED only when one of the others raised it
    assert flags & flag
    assert bool(flags & capi.FLAG_NOT_POLISHED) == bool((first[others] < S).any()) == bool(clean[8] & capi.FLAG_NOT_POLISHED)


def test_max_rounds_zero_verifies_only():
    """max_rounds = 0: an instance is carried exactly as long as the shifted start already passes; from a cold start
    nothing passes at step 0 on these inputs (a zero sequence is no optimum of a problem with targets)."""
    I, H, S = 2, 10, 4
    th, nlt = inputs("general", I, H, S)
    ins, nl = soa_inputs(th, nlt, N)
    u, x, q, st, it, first, ri, ro, flags = newton_host(I, H, S, ins, nl, rounds=0)
    assert not first.any() and np.all(st == -1) and not u.any() and not q.any() and flags == capi.FLAG_NOT_POLISHED
    # ... and a start whose shift is already the optimum is carried with 0 rounds: tight boxes (the optimum sits on
    # the bounds, so its last two rows agree and the shift reproduces it)
    I, H = 2, 4
    th, _ = inputs("batch", I, H, 1)
    ins, _ = soa_inputs(th, None, N)
    _, _, q8, _, _, first8, *_ = newton_host(I, H, 1, ins, None)
    start = np.concatenate([np.zeros((I, N)), q8[:(H - 1) * I]])
    u, x, q, st, it, first, ri, ro, flags = newton_host(I, H, 1, ins, None, rounds=0, controls=start.copy())
    w = composed_from(I, H, ins, start, rounds=0)
    print(f"max_rounds 0 from the shifted optimum: carried {int((first == 1).sum())}/{N}")
    assert q.tobytes() == w[0].tobytes() and st.tobytes() == w[1].tobytes()
    assert (first == 1).any() and (first == 0).any()
    assert np.all(st[0][first == 1] == 0) and np.all(ri[0][first == 1] <= TOL) and np.all(ri[0][first == 0] == 0.0)


# ---- 5. the code object ----------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_new_kernels_have_no_scratch_and_no_spills():
    """The step-loop kernel (both instantiations), gather, scatter and the flag merge are in the library; none has a
    private segment, a VGPR spill or a scratch instruction (read as tests/test_rollout_polish_host.py reads the fused
    step kernel), and the step-loop kernel keeps the fused step's occupancy: at most 128 / 96 VGPRs for I = 2 / 1
    (4 / 5 waves per SIMD of 512 registers, allocated in eights)."""
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    assert check_loop_scratch.offenders(lib, ["rollout_newton_kernel"]) == []
    seen, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            for name, body in check_loop_scratch.kernels(co):
                if "rollout_newton_" in name and not name.endswith(".kd"):
                    seen[name] = [t for _, t, _ in body if t.startswith("scratch_")]
            notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", co], capture_output=True,
                                   text=True, check=True).stdout
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                if "rollout_newton_" in fields.get(".name", ""):
                    meta[fields[".name"]] = fields
    assert len(meta) == 5, sorted(meta)
    for name, fields in meta.items():
        print(name, {k: fields[k] for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size",
                                            ".vgpr_spill_count", ".sgpr_spill_count")})
        assert int(fields[".private_segment_fixed_size"]) == 0 and int(fields[".vgpr_spill_count"]) == 0, fields
        assert fields[".uses_dynamic_stack"] == "false"
        if "rollout_newton_kernelILi2E" in name:
            assert int(fields[".vgpr_count"]) <= 128
        if "rollout_newton_kernelILi1E" in name:
            assert int(fields[".vgpr_count"]) <= 96
    assert len(seen) == 5, sorted(seen)
    assert all(not hits for hits in seen.values()), {k: len(v) for k, v in seen.items()}
