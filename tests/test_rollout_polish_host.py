"""CPU tests of the polished closed loop (tpc_mpc_rollout_polished, MpcSolver.rollout_polished): the symbol and the
ABI version, the entry's argument checks and its answer on a host-only handle (the closed loops run on the device
only), the code object of the fused polish + step kernel, and the CPU checker of the loop
(tests/model/mpc_rollout_polish_ref.py: oracle solve, polish, plant update per step) against the dense closed loop
on the polished sequences' active sets -- the statement "every step returned the optimum"."""
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
from trajectory_controller_amd import capi

NAMES = rd.NAMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Inputs of the optimality comparison: mpc_rollout_dense.batch(I, H, S, n, seed, with_nlt), solved at dlib's default
# eps 0.01, polished with tol 1e-9, 8 rounds.  Measured on the CPU (oracle + host polish), per case: unpolished
# (instance, step) pairs / pairs, and the largest deviation of the polished replay from the dense closed loop on its
# own active sets over the instances without an unpolished step:
#   (1, 4, 8, 40, 0, nlt)      0 / 320   2.0e-15        (unpolished replay at eps 0.01: 5.1e-2)
#   (2, 10, 10, 40, 1, nlt)    0 / 400   7.2e-14        (4.4e-2)
#   (2, 20, 6, 40, 2, no nlt)  1 / 240   2.3e-13        (9.5e-2)
#   (1, 20, 6, 40, 3, nlt)     0 / 240   1.85e-12       (3.7e-2)
# With mpc_polish_dense as the polisher the same four give 2.6e-15, 5.0e-14, 1.0e-12, 1.6e-12.
# The bound is 10x the largest of them, the convention of test_polish_host.py::test_library_against_checker.
CASES = [(1, 4, 8, 40, 0, True), (2, 10, 10, 40, 1, True), (2, 20, 6, 40, 2, False), (1, 20, 6, 40, 3, True)]
MEASURED = 1.85e-12
BOUND = 10 * MEASURED
CAP = 0.01          # at most 1 % of a batch's (instance, step) pairs may be unpolished
TOL, ROUNDS = 1e-9, 8


@functools.lru_cache(maxsize=None)
def polished_case(I, H, S, n, seed, with_nlt, polisher="host"):
    th, nlt = rd.batch(I, H, S, n, seed=seed, with_nlt=with_nlt)
    return th, nlt, rp.replay(I, H, S, th, nlt, tol=TOL, max_rounds=ROUNDS, polisher=polisher)


def test_symbol_and_abi_version():
    lib = capi.load_library()
    assert "tpc_mpc_rollout_polished" in capi.EXPORTS and hasattr(lib, "tpc_mpc_rollout_polished")
    assert lib.tpc_mpc_abi_version() == 5 == capi.ABI_VERSION
    with open(os.path.join(ROOT, "include", "tpc_mpc.h")) as f:
        assert "int tpc_mpc_rollout_polished(" in f.read()


@pytest.fixture
def host_handle():
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.tpc_mpc_create(capi.DEVICE_NONE, C.byref(h)) == 0
    yield h
    lib.tpc_mpc_destroy(h)


def _raw(h, H, I, S, n, tol=1e-9, rounds=8, dtype=capi.F64, mem=capi.HOST, q=True, ld=None):
    th, nlt = rd.batch(I, 4, 3, 3, seed=0)
    ins = {k: dense.soa(th[k], 3) for k in NAMES}
    p = capi.default_params(20, dtype=dtype)
    p.horizon = H
    ptr = lambda a: a.ctypes.data
    io = capi.GeneralIO(inputs=I, n=n, ld=n if ld is None else ld, A=ptr(ins["A"]), B=ptr(ins["B"]), C=ptr(ins["C"]),
                        Q=ptr(ins["Q"]), R=ptr(ins["R"]), lower=ptr(ins["lo"]), upper=ptr(ins["hi"]), x0=ptr(ins["x0"]),
                        targets=ptr(ins["targets"]))
    qq = capi.Polish(tol=tol, max_rounds=rounds)
    cu, cx = np.full((max(S, 1) * I, 3), 7.0), np.full((max(S, 1) * 2, 3), 7.0)
    flags = C.c_uint32(99)
    rc = capi.load_library().tpc_mpc_rollout_polished(h, C.byref(p), C.byref(io), S, None, C.byref(qq) if q else None,
                                                      ptr(cu), ptr(cx), None, None, C.byref(flags), mem, None)
    assert np.all(cu == 7.0) and np.all(cx == 7.0)     # nothing is written on an error
    return rc


def test_argument_errors_come_before_the_device(host_handle):
    lib = capi.load_library()
    I, H, S, n = 2, 4, 3, 3
    msg = lambda: lib.tpc_mpc_last_error(host_handle)
    assert _raw(host_handle, H, I, S, n, q=False) == 1 and b"polish" in msg()
    for kw in (dict(tol=0.0), dict(tol=-1e-9), dict(tol=np.nan), dict(rounds=-1)):
        assert _raw(host_handle, H, I, S, n, **kw) == 1 and b"tol > 0" in msg(), kw
    assert _raw(host_handle, H, I, S, n, dtype=capi.F32) == 1 and b"fp64" in msg()
    assert _raw(host_handle, H, I, -1, n) == 1 and b"steps" in msg()
    assert _raw(host_handle, H, I, (1 << 24) + 1, n) == 1 and b"steps" in msg()
    assert _raw(host_handle, 65, I, S, n) == 4
    assert _raw(host_handle, H, 3, S, n) == 1
    assert _raw(host_handle, H, I, S, n, ld=n - 1) == 1
    # valid arguments: the closed loops have no host path
    for mem in (capi.HOST, capi.DEVICE):
        assert _raw(host_handle, H, I, S, n, mem=mem) == 6 and b"host-only" in msg()
    # ... and the existing closed loops answer a host-only handle as before
    p = capi.default_params(4)
    io = capi.GeneralIO(inputs=I, n=n, ld=n)
    assert lib.tpc_mpc_rollout(host_handle, C.byref(p), C.byref(io), S, None, None, None, None, None, capi.HOST,
                               None) == 6


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_fused_step_kernel_has_no_scratch():
    """Both instantiations of the fused polish + step kernel are in the library and touch no scratch memory: no
    scratch instruction in their bodies (read as tests/test_rollout_grad_host.py reads the backward kernel) and a
    zero private segment in the code object's metadata."""
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_loop_scratch
    lib = os.path.join(ROOT, "trajectory_controller_amd", "lib", "libtpc_mpc.so")
    assert check_loop_scratch.offenders(lib, ["rollout_polish_step_kernel"]) == []
    seen, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in check_loop_scratch.device_objects(lib, tmp):
            for name, body in check_loop_scratch.kernels(co):
                if "rollout_polish_step_kernel" in name and not name.endswith(".kd"):
                    seen[name] = [t for _, t, _ in body if t.startswith("scratch_")]
            notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", co], capture_output=True,
                                   text=True, check=True).stdout
            for block in notes.split("- .agpr_count")[1:]:     # one block of fields per kernel
                fields = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", block, flags=re.M))
                if "rollout_polish_step_kernel" in fields.get(".name", ""):
                    meta[fields[".name"]] = fields
    assert len(meta) == 2, sorted(meta)
    for name, fields in meta.items():
        print(name, {k: fields[k] for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size",
                                            ".vgpr_spill_count", ".sgpr_spill_count")})
        assert int(fields[".private_segment_fixed_size"]) == 0 and int(fields[".vgpr_spill_count"]) == 0, fields
        assert fields[".uses_dynamic_stack"] == "false"
    assert len(seen) == 2, sorted(seen)
    assert all(not hits for hits in seen.values()), {k: len(v) for k, v in seen.items()}


@pytest.mark.parametrize("I,H,S,n,seed,with_nlt", CASES)
def test_polished_replay_is_the_dense_closed_loop(I, H, S, n, seed, with_nlt):
    """Every step returned the optimum: the polished replay's u0 and states equal the dense closed loop evaluated on
    the polished sequences' active sets, within BOUND; the unpolished replay at eps 0.01 misses the same bound by
    orders of magnitude."""
    th, nlt, (u0, xs, sq, st, it, ri, ro) = polished_case(I, H, S, n, seed, with_nlt)
    share = float((st < 0).mean())
    whole = (st >= 0).all(axis=1)
    dev = rp.deviation_from_optimum(I, H, S, th, nlt, u0, xs, sq)
    print(f"I={I} H={H} S={S}: unpolished pairs {int((st < 0).sum())}/{st.size}, largest deviation "
          f"{dev[whole].max():.3e} (bound {BOUND:.3e})")
    assert share <= CAP, share
    assert np.all(ro[st >= 0] <= TOL) and np.all(ro <= ri)
    assert dev[whole].max() <= BOUND, dev[whole].max()
    # what the feature buys: the loop as it is today, at the same eps
    u0n, xsn, sqn, _, itn, _, _ = rp.replay(I, H, S, th, nlt, polisher=None)
    for i in range(0, n, 7):   # polisher=None is mpc_rollout_dense.replay, bit for bit
        a, b, c, d = rd.replay(I, H, S, {k: th[k][i] for k in NAMES}, None if nlt is None else nlt[i])
        assert np.array_equal(a, u0n[i]) and np.array_equal(b, xsn[i]) and np.array_equal(c, sqn[i])
        assert np.array_equal(d, itn[i])
    devn = rp.deviation_from_optimum(I, H, S, th, nlt, u0n, xsn, sqn)
    print(f"    unpolished replay: largest deviation {devn.max():.3e}, share of instances over the bound "
          f"{float((devn > BOUND).mean()):.2f}")
    assert devn.max() > 1e3 * BOUND, devn.max()   # a residual of 0.01 is not a rounding: measured 3.7e-2 .. 9.5e-2


@pytest.mark.parametrize("I,H,S,n,seed,with_nlt", CASES[:2])
def test_the_two_polishers_give_the_same_loop(I, H, S, n, seed, with_nlt):
    """The library's rule on the host-only handle and the dense restatement, each carried through the whole loop:
    both reach the optimum of every step, so the loops agree to the bound (twice: each is within BOUND of it)."""
    th, nlt, (u0, xs, sq, st, *_) = polished_case(I, H, S, n, seed, with_nlt)
    _, _, (du0, dxs, dsq, dst, *_) = polished_case(I, H, S, n, seed, with_nlt, polisher="dense")
    both = (st >= 0).all(axis=1) & (dst >= 0).all(axis=1)
    assert both.mean() >= 0.9
    assert np.abs(u0 - du0)[both].max() <= 2 * BOUND and np.abs(xs - dxs)[both].max() <= 2 * BOUND
