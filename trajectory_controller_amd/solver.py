"""Host-side handle over the C ABI: `MpcSolver`.

Mirrors the reference's operator surface for this path -- dlib::mpc's constructor knobs
(epsilon, max_iterations; mpc.h:187-214), `mpcControllerTobi(v, delta_y, delta_phi)`
(src/trajectory_point_follower.cpp:301-389) -- for one instance or a batch.  Arrays may be numpy
(host memory: the library stages them) or torch tensors on the GPU (device pointers are handed to
the library as they are, launches go to torch's current stream).  torch is used for device memory
and streams only; all arithmetic is in the HIP kernels behind libtpc_mpc.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import capi
from ._arrays import LAST, Arrays

COMPACT_PARAM_NAMES = capi.COMPACT_PARAM_NAMES   # the order of solve_batch_compact_exact_backward's "params"
_I32 = np.int32


def _rows(I: int, H: int, steps: int = 0) -> dict:
    """Rows of every component-major general-form array [rows, n], by the name its gradient / tangent goes by."""
    return {"A": 4, "B": 2 * I, "C": 2, "Q": 2, "R": I, "lower": I, "upper": I, "x0": 2, "targets": 2 * H,
            "new_last_targets": 2 * steps, "kkt_residual": 1, "Ap": 4, "Bp": 2 * I, "Cp": 2, "disturbance": 2 * steps}


def _check_names(kind, given, allowed):
    unknown = set(given) - set(allowed)
    if unknown:
        raise ValueError(f"unknown {kind} names {sorted(unknown)}")


def _directions(tangents, ndim, expected):
    """K of a dict of tangent arrays: an array of ndim(name) dimensions leads with K, one with a dimension fewer is
    K = 1, and all agree"""
    K = None
    for name, t in tangents.items():
        k = 1 if t.ndim == ndim(name) - 1 else t.shape[0] if t.ndim == ndim(name) else None
        if k is None or (K is not None and k != K):
            raise ValueError(f"tangent {name!r}: expected {expected} with one K for all")
        K = k
    return K


class MpcSolver:
    """One tpc_mpc_handle bound to a HIP device (device=None: host-only, TPC_MPC_DEVICE_NONE).  Not thread-safe (like the handle)."""

    def __init__(self, horizon: int = 20, device: int = 0, dtype: str = "f64", algo: str = "auto",
                 **params):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        device = capi.DEVICE_NONE if device is None else int(device)   # None: a host-only handle (solve_one only, no GPU touched)
        rc = self._lib.tpc_mpc_create(device, C.byref(self._h))
        if rc != capi.OK:
            raise capi.TpcMpcError(rc, self._lib.tpc_mpc_last_error(None).decode())
        self.device = device
        self.dtype = {"f64": capi.F64, "f32": capi.F32}[dtype]
        self.algo = {"auto": capi.ALGO_AUTO, "wave": capi.ALGO_WAVE, "lane": capi.ALGO_LANE,
                     "lane_fma": capi.ALGO_LANE_FMA, "group": capi.ALGO_GROUP}[algo]
        self.params = capi.default_params(horizon, self.dtype, self.algo, **params)
        self.last_flags = 0
        self.rank, self.world = 0, 1     # a handle without a communicator is a world of one

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.tpc_mpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def horizon(self) -> int:
        return self.params.horizon

    def _check(self, rc: int):
        if rc != capi.OK:
            raise capi.TpcMpcError(rc, self._lib.tpc_mpc_last_error(self._h).decode())

    def _params(self, **over) -> capi.Params:
        if not over:
            return self.params
        p = capi.Params.from_buffer_copy(self.params)
        for k, val in over.items():
            if k in ("lower", "upper"):
                getattr(p, k)[0], getattr(p, k)[1] = float(val[0]), float(val[1])
            else:
                setattr(p, k, val)
        return p

    # -- what every array-taking call shares --------------------------------------------------------
    def _run(self, entry, p, ar, *args, want_flags=True, mem=True):
        """entry(handle, &p, *args, &flags, [mem,] stream), then last_flags: the end of every batch call.
        want_flags=False passes a null flags_out (a DEVICE call then stays asynchronous) and leaves last_flags at 0."""
        flags = C.c_uint32(0)
        where = (ar.mem, ar.stream) if mem else (ar.stream,)
        self._check(entry(self._h, C.byref(p), *args, C.byref(flags) if want_flags else None, *where))
        self.last_flags = flags.value

    @staticmethod
    def _general(A, R, inputs, dtype=np.float64):
        """(Arrays, I) of a general-form call: n is A's last dimension, I the rows of R unless given"""
        return Arrays(A, LAST, dtype), inputs or np.shape(R)[0]

    @staticmethod
    def _io(ar, I, H, model, controls=None, v_state=None, u0=None, iters=None, match="shape"):
        """capi.GeneralIO of the nine model arrays (read), controls / v_state (updated in place) and the outputs u0 /
        iters that ar.new made"""
        A, B, Cc, Q, R, lower, upper, x0, targets = ar.read_rows(model, (4, 2 * I, 2, 2, I, I, I, 2, 2 * H), match)
        return capi.GeneralIO(inputs=I, n=ar.n, ld=ar.n, A=A, B=B, C=Cc, Q=Q, R=R, lower=lower, upper=upper, x0=x0,
                              targets=targets, controls_inout=ar.update(controls, H * I),
                              v_inout=ar.update(v_state, H * I), u0=ar.addr(u0), iters=ar.addr(iters))

    # -- measurement ------------------------------------------------------------------------------
    def set_profiling(self, enable: bool = True):
        self._check(self._lib.tpc_mpc_set_profiling(self._h, int(enable)))

    def last_kernel_times(self):
        """(first_kernel_ms, second_kernel_ms, algo) of the last solve; waits for it."""
        a, b, algo = C.c_double(), C.c_double(), C.c_int()
        self._check(self._lib.tpc_mpc_last_kernel_times(self._h, C.byref(a), C.byref(b), C.byref(algo)))
        return a.value, b.value, algo.value

    def last_lane_stats(self):
        """(wave_iterations, refill_blocks) of the last LANE solve; synchronises the device."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.tpc_mpc_last_lane_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- the call being replaced ------------------------------------------------------------------
    def mpc_controller_tobi(self, v: float, delta_y: float, delta_phi: float, **over):
        """mpcControllerTobi(v, delta_y, delta_phi, &front, &rear): returns (front, rear)."""
        f, r = C.c_double(), C.c_double()
        self._check(self._lib.tpc_mpc_solve_one(self._h, C.byref(self._params(**over)), float(v),
                                                float(delta_y), float(delta_phi), C.byref(f),
                                                C.byref(r)))
        return f.value, r.value

    solve_one = mpc_controller_tobi

    def last_solve_one_flags(self):
        """(flags, iterations) of the last solve_one (tpc_mpc_last_flags): capi.FLAG_NONFINITE when the speed
        or the target was NaN / Inf (the call returned dlib's untouched start point), capi.FLAG_MAX_ITER when
        max_iter cut the solve off."""
        f, it = C.c_uint32(), C.c_int32()
        self._check(self._lib.tpc_mpc_last_flags(self._h, C.byref(f), C.byref(it)))
        return f.value, it.value

    def set_option(self, option: int, value: int):
        """tpc_mpc_set_option: capi.OPT_WAVE_GROUP (0 auto, 1, 2, 4), capi.OPT_MAILBOX_HOST (0 / 1)."""
        self._check(self._lib.tpc_mpc_set_option(self._h, int(option), int(value)))

    def set_resident(self, idle_timeout_us: int = 20000):
        """solve_one's resident wavefront: idle timeout in microseconds, <= 0 turns it off
        (tpc_mpc_set_resident)."""
        self._check(self._lib.tpc_mpc_set_resident(self._h, int(idle_timeout_us)))

    @staticmethod
    def build_info() -> str:
        return capi.load_library().tpc_mpc_build_info().decode()

    # -- batches ----------------------------------------------------------------------------------
    def reserve(self, n: int, host: bool = False, **over):
        """Allocate the device scratch for compact batches of up to n instances now
        (tpc_mpc_reserve), so that no later solve allocates -- needed when several batches are kept
        in flight on different streams, because a device allocation synchronises all of them."""
        p = self._params(**over)
        self._check(self._lib.tpc_mpc_reserve(self._h, C.byref(p), int(n), capi.HOST if host else capi.DEVICE))

    def set_work_hint(self, hint):
        """Queue-order hint for the next batch solve of the same size (experimental: tpc_mpc_x_set_work_hint,
        csrc/tpc_mpc_experimental.h):
        per-instance iteration-count estimates, typically the `iters` of the previous cycle.
        int32 numpy array (copied) or CUDA tensor (read by the next solve; keep it alive until
        then).  None clears.  Never changes a result, only the order lanes pick instances up."""
        if hint is None:
            self._check(self._lib.tpc_mpc_x_set_work_hint(self._h, None, 0, capi.HOST))
            self._hint_ref = None
        else:
            ar = Arrays(hint, None, _I32)
            self._check(self._lib.tpc_mpc_x_set_work_hint(self._h, ar.read(hint, match="length"), ar.n, ar.mem))
            if ar.mem == capi.DEVICE:
                self._hint_ref = hint

    QUEUE_KEYS = ("lambda", "table", "hint")

    def set_queue_key(self, table: bool = True):
        """LANE_FMA, fp64, N = 20 with the reference controller's parameters: order the work queue by the iteration count
        csrc/mpc_queue_key_table.h predicts (True, the default) or by lambda like everything else (False).  Experimental
        (tpc_mpc_x_set_queue_key): for A/B runs and tests; never changes a result."""
        self._check(self._lib.tpc_mpc_x_set_queue_key(self._h, int(bool(table))))

    def last_queue_key(self) -> str:
        """What ordered the work queue of the last compact batch: "lambda", "table" or "hint" (tpc_mpc_x_last_queue_key)."""
        k = C.c_int()
        self._check(self._lib.tpc_mpc_x_last_queue_key(self._h, C.byref(k)))
        return self.QUEUE_KEYS[k.value]

    def solve_batch_compact(self, v, delta_y, delta_phi, want_iters: bool = False,
                            want_flags: bool = True, out=None, **over):
        """n independent mpcControllerTobi calls.  Returns (front, rear[, iters])."""
        p = self._params(**over)
        ar = Arrays(v, None, p.dtype, like=True)
        ins = ar.read_rows((v, delta_y, delta_phi), None, "length")
        if out is None or ar.mem == capi.HOST:     # (a HOST call has always returned fresh arrays, whatever out= is)
            front, rear = ar.new(), ar.new()
            outs = (ar.addr(front), ar.addr(rear))
        else:
            front, rear = out
            outs = (ar.update(front, match="length"), ar.update(rear, match="length"))
        iters = ar.new(dtype=_I32) if want_iters else None
        self._run(self._lib.tpc_mpc_solve_batch_compact, p, ar, ar.n, *ins, *outs, ar.addr(iters),
                  want_flags=want_flags or ar.mem == capi.HOST)   # (a HOST call is synchronous: it always reports)
        return (front, rear, iters) if want_iters else (front, rear)

    def solve_batch_compact_exact(self, v, delta_y, delta_phi, tol: float = 1e-9, max_rounds: int = 16,
                                  fallback: str = "solve", want_status: bool = True, want_sequence: bool = False,
                                  want_residuals: bool = False, params_rows=None, start=None, **over):
        """n independent mpcControllerTobi calls answered with the verified optimum instead of dlib's eps-0.01 point
        (tpc_mpc_solve_batch_compact_exact), fp64 only.

        Every instance runs the polish's Newton rounds from U = 0 on the reference controller's model in one launch;
        fallback="solve" then runs the first-order solve and the polish for the instances the rounds did not verify
        (p's eps / max_iter / algo), fallback="none" returns (0, 0) with status -1 for them and is what a host-only
        handle (device=None) serves.  Arrays as in solve_batch_compact (numpy: HOST memory, CUDA tensors: DEVICE memory
        on the current stream).  Returns (front, rear[, sequence], status, fell_back[, residual_in, residual_out]):
        sequence [2H, n] with want_sequence; status int32 [n] = the Newton rounds used or -1; fell_back int32 [n] = 1
        where the solve ran (None with fallback="none"); the residuals with want_residuals.  Sets last_flags
        (FLAG_NOT_POLISHED if an instance is left unverified, FLAG_NONFINITE for a NaN / Inf input).
        want_status=False returns None for status and fell_back; with fallback="none" it also leaves last_flags at 0
        and keeps a DEVICE call asynchronous (fallback="solve" synchronises between its phases anyway and always
        reports the flags).  want_residuals is for checks: the polish's two residual rows.  max_rounds=16: from 8 to
        16 halves the share that falls back, 32 gains little.
        params_rows ([10, n] fp64, numpy or a contiguous CUDA tensor like v; rows in the order of
        COMPACT_PARAM_NAMES) gives every instance its own weights, step_size, wheelbase and bounds
        (tpc_mpc_solve_batch_compact_exact_rows): the solver's ten model values are then not read, an instance with an
        invalid column returns (0, 0) with status -1 and raises FLAG_NONFINITE or FLAG_BAD_MODEL, and the fallback
        expands the unverified instances with their own values.  None is the shared entry.
        start ([2H, n] fp64, numpy or a contiguous CUDA tensor like v; the layout of `sequence`) warm-starts the Newton
        rounds (tpc_mpc_solve_batch_compact_exact_from, with or without params_rows): instance k begins at its column,
        clamped to its bounds -- in a fitting loop, the `sequence` the previous step returned.  A column with a NaN or
        an Inf means "no start for this one" and is the cold start, as a column of zeros is; the fallback stays cold.
        None is the cold call above.
        Its derivative is solve_batch_compact_exact_backward (autograd: mpc_compact_exact)."""
        p = self._params(**over)
        H = p.horizon
        ar = Arrays(v)
        rd = ar.read
        vectors = ar.read_rows((v, delta_y, delta_phi), None, "length")
        front, rear = ar.new(), ar.new()
        seq = ar.new(2 * H) if want_sequence else None
        status = ar.new(dtype=_I32) if want_status else None
        fell = ar.new(dtype=_I32) if want_status and fallback != "none" else None
        rin, rout = (ar.new(), ar.new()) if want_residuals else (None, None)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=ar.addr(status),
                        residual_in=ar.addr(rin), residual_out=ar.addr(rout))
        if start is not None:
            entry = self._lib.tpc_mpc_solve_batch_compact_exact_from
            model = (rd(params_rows, len(COMPACT_PARAM_NAMES)), rd(start, 2 * H))
        elif params_rows is not None:
            entry, model = self._lib.tpc_mpc_solve_batch_compact_exact_rows, (rd(params_rows, len(COMPACT_PARAM_NAMES)),)
        else:
            entry, model = self._lib.tpc_mpc_solve_batch_compact_exact, ()
        self._run(entry, p, ar, ar.n, *vectors, *model, C.byref(q), capi.NEWTON_FALLBACKS[fallback], ar.addr(front),
                  ar.addr(rear), ar.addr(seq), ar.addr(fell), want_flags=want_status or fallback != "none")
        out = (front, rear) + ((seq,) if want_sequence else ()) + (status, fell)
        return out + ((rin, rout) if want_residuals else ())

    COMPACT_GRAD_NAMES = ("v", "delta_y", "delta_phi", "params", "params_rows", "kkt_residual")

    def solve_batch_compact_exact_backward(self, v, delta_y, delta_phi, sequence, grad_front=None, grad_rear=None,
                                           grad_sequence=None, status=None,
                                           want=("v", "delta_y", "delta_phi", "params"), want_flags: bool = True,
                                           params_rows=None, **over):
        """Backward pass of solve_batch_compact_exact (tpc_mpc_solve_batch_compact_exact_backward), fp64 only.

        Arrays as in solve_batch_compact_exact (numpy: HOST memory, CUDA tensors: DEVICE memory on the current stream):
        v, delta_y, delta_phi [n], `sequence` [2H, n] as want_sequence returns it, `status` (int32 [n], optional: an
        instance with a negative status is excluded).  The incoming gradient is grad_front, grad_rear [n] and
        grad_sequence [2H, n], each optional (zero).  Returns a dict keyed by `want`: "v", "delta_y", "delta_phi" [n],
        "params" [10] (the gradient of the shared parameters in the order of COMPACT_PARAM_NAMES, summed over the
        batch on the device in a fixed order, the same bytes on every call), "params_rows" [10, n] (per instance) and
        "kkt_residual" [n].  Excluded instances (negative status, non-finite data: last_flags) get zeros and add
        nothing to "params"; want_flags=False leaves last_flags at 0 and keeps a DEVICE call asynchronous.
        With params_rows ([10, n], as solve_batch_compact_exact takes it: tpc_mpc_solve_batch_compact_exact_rows_backward)
        "params_rows" is the gradient with respect to each instance's own ten parameters and "params" their sum."""
        p = self._params(**over)
        H = p.horizon
        _check_names("gradient", want, self.COMPACT_GRAD_NAMES)
        ar = Arrays(v)
        NP = len(COMPACT_PARAM_NAMES)
        out = {k: ar.new(NP, per_instance=False) if k == "params" else ar.new(NP) if k == "params_rows" else ar.new()
               for k in self.COMPACT_GRAD_NAMES if k in want}
        to = {k: ar.addr(a) for k, a in out.items()}
        g = capi.CompactGrad(grad_front=ar.read(grad_front), grad_rear=ar.read(grad_rear),
                             grad_sequence=ar.read(grad_sequence, 2 * H), dv=to.get("v"), ddelta_y=to.get("delta_y"),
                             ddelta_phi=to.get("delta_phi"), dparams_rows=to.get("params_rows"),
                             dparams=to.get("params"), kkt_residual=to.get("kkt_residual"))
        if params_rows is None:
            entry, rows = self._lib.tpc_mpc_solve_batch_compact_exact_backward, ()
        else:
            entry, rows = self._lib.tpc_mpc_solve_batch_compact_exact_rows_backward, (ar.read(params_rows, NP),)
        self._run(entry, p, ar, ar.n, ar.read(v), ar.read(delta_y), ar.read(delta_phi), *rows,
                  ar.read(sequence, 2 * H), ar.read(status, dtype=_I32), C.byref(g), want_flags=want_flags)
        return out

    COMPACT_TANGENT_NAMES = ("v", "delta_y", "delta_phi", "params", "params_rows")

    def solve_batch_compact_exact_forward(self, v, delta_y, delta_phi, sequence, tangents, status=None,
                                          params_rows=None, want_sequence: bool = False, want_flags: bool = True,
                                          **over):
        """Forward mode of solve_batch_compact_exact (tpc_mpc_solve_batch_compact_exact_forward), fp64 only: the
        directional derivatives of (front, rear) -- with want_sequence of the whole sequence -- along K directions,
        taken at `sequence` [2H, n] as want_sequence of the forward returns it.  K directions in one call are K columns
        of the per-instance Jacobian: what Gauss-Newton and Levenberg-Marquardt fits of a few parameters need.

        Arrays as in solve_batch_compact_exact_backward (numpy: HOST memory, CUDA tensors: DEVICE memory on the
        current stream); `status` (int32 [n], optional) excludes the instances with a negative status.  `tangents`
        maps "v", "delta_y", "delta_phi" to arrays [K, n] ([n]: K = 1), and the parameters' tangent, in the order of
        COMPACT_PARAM_NAMES, either "params" [K, 10] ([10]: K = 1; the ten shared parameters, params_rows=None only;
        a CUDA tensor in a DEVICE call) or "params_rows" [K, 10, n] ([10, n]: K = 1; with params_rows only).  A missing
        name is a zero tangent.  Returns (tfront [K, n], trear [K, n]), and tsequence [K, 2H, n] with want_sequence;
        a flagged (direction, instance) pair and an excluded instance get zeros (last_flags).  want_flags=False leaves
        last_flags at 0 and keeps a DEVICE call asynchronous."""
        p = self._params(**over)
        H = p.horizon
        _check_names("tangent", tangents, self.COMPACT_TANGENT_NAMES)
        tangents = {k: t for k, t in tangents.items() if t is not None}
        if not tangents:
            raise ValueError("tangents is empty: give at least one direction array")
        if "params" in tangents and params_rows is not None:
            raise ValueError('"params" is the shared parameters\' tangent: with params_rows give "params_rows"')
        if "params_rows" in tangents and params_rows is None:
            raise ValueError('"params_rows" needs params_rows')
        K = _directions(tangents, lambda name: 3 if name == "params_rows" else 2,
                        "a leading K (or none for K = 1)")
        ar = Arrays(v)
        NP = len(COMPACT_PARAM_NAMES)
        at = {name: ar.read(t, K * NP, None, "elems") if name == "params"
              else ar.read(t, K * NP if name == "params_rows" else K, None, "loose") for name, t in tangents.items()}
        tan = capi.CompactTangents(directions=K, reserved=0, tv=at.get("v"), tdelta_y=at.get("delta_y"),
                                   tdelta_phi=at.get("delta_phi"), tparams=at.get("params"),
                                   tparams_rows=at.get("params_rows"))
        tfront, trear = ar.new(K), ar.new(K)
        tseq = ar.new(K, 2 * H) if want_sequence else None
        self._run(self._lib.tpc_mpc_solve_batch_compact_exact_forward, p, ar, ar.n, ar.read(v), ar.read(delta_y),
                  ar.read(delta_phi), ar.read(params_rows, NP), ar.read(sequence, 2 * H), ar.read(status, dtype=_I32),
                  C.byref(tan), ar.addr(tfront), ar.addr(trear), ar.addr(tseq), want_flags=want_flags)
        return (tfront, trear, tseq) if want_sequence else (tfront, trear)

    def solve_batch_compact_mixed(self, horizons, v, delta_y, delta_phi, want_iters: bool = False, **over):
        """Mixed-horizon batch (BASELINE config 5): instance k is solved with horizon horizons[k]
        (tpc_mpc_solve_batch_compact_mixed: binned by horizon on the device, one launch sequence per
        bin, results back in the caller's order).  Arrays as in solve_batch_compact; `horizons` is an
        integer array/tensor of the same length."""
        p = self._params(**over)
        ar = Arrays(v, None, p.dtype, like=True)
        front, rear = ar.new(), ar.new()
        iters = ar.new(dtype=_I32) if want_iters else None
        self._run(self._lib.tpc_mpc_solve_batch_compact_mixed, p, ar, ar.n,
                  ar.read(horizons, dtype=_I32, match="length", convert=True),
                  *ar.read_rows((v, delta_y, delta_phi), None, "length"), ar.addr(front), ar.addr(rear), ar.addr(iters))
        return (front, rear, iters) if want_iters else (front, rear)

    # -- sharding over the GPUs of a node ----------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte communicator id (rank 0 makes it, the host hands it to every rank)."""
        lib = capi.load_library()
        buf = (C.c_char * capi.COMM_ID_BYTES)()
        rc = lib.tpc_mpc_comm_unique_id(buf, capi.COMM_ID_BYTES)
        if rc != capi.OK:
            raise capi.TpcMpcError(rc, lib.tpc_mpc_last_error(None).decode())
        return bytes(buf)

    def comm_test_mode(self, force_communicator: bool, force_ragged: bool = False):
        """Test hook (tpc_mpc_comm_test_mode): a real one-rank communicator / the ragged exchange on one GPU."""
        self._check(self._lib.tpc_mpc_comm_test_mode(self._h, int(force_communicator), int(force_ragged)))

    def comm_init(self, comm_id: bytes, rank: int, world: int):
        """Join the job's RCCL communicator as `rank` of `world` (tpc_mpc_comm_init_rank)."""
        buf = (C.c_char * capi.COMM_ID_BYTES).from_buffer_copy(bytes(comm_id).ljust(capi.COMM_ID_BYTES, b"\0"))
        self._check(self._lib.tpc_mpc_comm_init_rank(self._h, buf, capi.COMM_ID_BYTES, int(rank), int(world)))
        self.rank, self.world = int(rank), int(world)

    def solve_batch_compact_sharded(self, n_total: int, v_shard, dy_shard, dphi_shard, out=None,
                                    want_iters: bool = False, want_flags: bool = False, split: str = "block", **over):
        """This rank's shard of a batch of n_total, then the all-gather of the control outputs over RCCL
        (tpc_mpc_solve_batch_compact_sharded_split).  split "block": the shard is the contiguous block of shard_range;
        "interleaved": instances rank, rank + world, ... compacted (shard_map).  Device tensors; returns full-size
        (front, rear) in instance order under either split."""
        p = self._params(**over)
        first, count, stride = C.c_int64(), C.c_int64(), C.c_int64()
        self._lib.tpc_mpc_shard_map(int(n_total), self.rank, self.world, capi.SPLITS[split], C.byref(first), C.byref(count),
                                    C.byref(stride))
        ar = self._device_only(Arrays(v_shard, count.value, p.dtype))   # this rank's count.value instances
        shard = [ar.read(t, match="length") for t in (v_shard, dy_shard, dphi_shard)]
        front, rear = out if out is not None else (ar.new(int(n_total), per_instance=False),
                                                   ar.new(int(n_total), per_instance=False))
        iters = ar.new(dtype=_I32) if want_iters else None
        self._run(self._lib.tpc_mpc_solve_batch_compact_sharded_split, p, ar, int(n_total), capi.SPLITS[split], *shard,
                  front.data_ptr(), rear.data_ptr(), ar.addr(iters), want_flags=want_flags, mem=False)
        return (front, rear, iters) if want_iters else (front, rear)

    def shard_range(self, n_total: int):
        """(first, count) of this rank's contiguous block of a batch of n_total (tpc_mpc_shard_range)."""
        first, count = C.c_int64(), C.c_int64()
        self._lib.tpc_mpc_shard_range(int(n_total), self.rank, self.world, C.byref(first), C.byref(count))
        return first.value, count.value

    def shard_map(self, n_total: int, split: str = "block"):
        """(first, count, stride): element j of this rank's shard is instance first + j * stride (tpc_mpc_shard_map)."""
        first, count, stride = C.c_int64(), C.c_int64(), C.c_int64()
        self._lib.tpc_mpc_shard_map(int(n_total), self.rank, self.world, capi.SPLITS[split], C.byref(first), C.byref(count),
                                    C.byref(stride))
        return first.value, count.value, stride.value

    def gather_shards(self, n_total: int, *rows, split: str = "block"):
        """The exchange by itself, for any other entry a host shards (mixed horizons, follow, rollout): `rows` are FULL-size
        1-D CUDA tensors (or the rows of 2-D ones) of n_total elements of 4 or 8 bytes each, of which this rank has written
        its block [first, first + count) -- afterwards every rank holds all of every row (tpc_mpc_gather_shards_split).
        split "interleaved": the rank's shard sits compacted in the row's first `count` elements instead."""
        import torch
        flat = []
        for t in rows:
            if not (t.is_cuda and t.is_contiguous() and t.shape[-1] == n_total and t.element_size() in (4, 8)):
                raise ValueError("rows must be contiguous CUDA tensors whose last dimension is n_total, 4- or 8-byte elements")
            flat.extend(t.reshape(-1, n_total).unbind(0))
        if not flat:
            return
        es = flat[0].element_size()
        if any(r.element_size() != es for r in flat):
            raise ValueError("one call exchanges rows of one element size")
        table = (C.c_void_p * len(flat))(*[r.data_ptr() for r in flat])
        stream = torch.cuda.current_stream(flat[0].device).cuda_stream
        self._check(self._lib.tpc_mpc_gather_shards_split(self._h, int(n_total), capi.SPLITS[split], table, len(flat), es,
                                                          C.c_void_p(stream)))

    def solve_batch_general_sharded(self, A, B, Cc, Q, R, lower, upper, x0, targets, inputs: Optional[int] = None,
                                    want_iters: bool = False, **over):
        """The general form sharded (tpc_mpc_solve_batch_general_sharded): FULL-size component-major CUDA tensors
        [rows, n_total] on every rank (only this rank's block of columns has to be filled); solves that block in
        place and all-gathers the rows of u0 over RCCL.  Returns the full u0[I, n_total] (and this rank's iters)."""
        p = self._params(**over)
        ar, I = self._general(A, R, inputs, p.dtype)
        self._device_only(ar)
        u0 = ar.new(I)
        iters = ar.new(dtype=_I32).zero_() if want_iters else None
        io = self._io(ar, I, p.horizon, (A, B, Cc, Q, R, lower, upper, x0, targets), u0=u0, iters=iters)
        self._run(self._lib.tpc_mpc_solve_batch_general_sharded, p, ar, C.byref(io), mem=False)
        return (u0, iters) if want_iters else u0

    def solve_batch_general(self, A, B, Cc, Q, R, lower, upper, x0, targets, controls=None,
                            v_state=None, inputs: Optional[int] = None, want_iters: bool = False,
                            **over):
        """n independent dlib::mpc<2,I,H> controllers: ctor + set_target(t) + operator()(x0).

        Arrays are component-major (SoA): A[4,n] B[2I,n] C[2,n] Q[2,n] R[I,n] lower[I,n] upper[I,n]
        x0[2,n] targets[2H,n]; controls / v_state [H*I, n] are updated in place when given.
        Returns (u0[I,n][, iters])."""
        p = self._params(**over)
        ar, I = self._general(A, R, inputs, p.dtype)
        u0 = ar.new(I)
        iters = ar.new(dtype=_I32) if want_iters else None
        io = self._io(ar, I, p.horizon, (A, B, Cc, Q, R, lower, upper, x0, targets), controls, v_state, u0, iters)
        self._run(self._lib.tpc_mpc_solve_batch_general, p, ar, C.byref(io))
        return (u0, iters) if want_iters else u0

    def polish_batch_general(self, A, B, Cc, Q, R, lower, upper, x0, targets, controls, tol: float = 1e-9,
                             max_rounds: int = 8, want_status: bool = True, inputs: Optional[int] = None, **over):
        """Polish solved sequences to the exact optimum (tpc_mpc_polish_batch_general), fp64 only.

        Arrays as in solve_batch_general (numpy: HOST memory, CUDA torch tensors: DEVICE memory on the current stream);
        `controls` [H*I, n] -- what solve_batch_general left there -- is updated in place: an instance that reaches
        residual <= tol (dlib's eps) within max_rounds safeguarded Newton rounds gets the verified optimum, every other
        one keeps its bits.  Returns (controls, status, residual_in, residual_out) with status int32 [n] = rounds
        used or -1, and sets last_flags (FLAG_NOT_POLISHED if any instance was left); want_status=False returns
        controls alone, leaves last_flags at 0 and keeps a DEVICE call asynchronous."""
        p = self._params(**over)
        ar, I = self._general(A, R, inputs)
        status = ar.new(dtype=_I32) if want_status else None
        rin, rout = (ar.new(), ar.new()) if want_status else (None, None)
        io = self._io(ar, I, p.horizon, (A, B, Cc, Q, R, lower, upper, x0, targets), controls)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=ar.addr(status),
                        residual_in=ar.addr(rin), residual_out=ar.addr(rout))
        self._run(self._lib.tpc_mpc_polish_batch_general, p, ar, C.byref(io), C.byref(q), want_flags=want_status)
        return (controls, status, rin, rout) if want_status else controls

    GRAD_NAMES = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "kkt_residual")

    def solve_batch_general_backward(self, A, B, Cc, Q, R, lower, upper, x0, targets, controls, grad_controls,
                                     inputs: Optional[int] = None, want=GRAD_NAMES, want_flags: bool = True, **over):
        """Backward pass of solve_batch_general (tpc_mpc_solve_batch_general_backward), fp64 only.

        Arrays as in solve_batch_general (numpy: HOST memory, CUDA torch tensors: DEVICE memory on the current stream);
        `controls` [H*I, n] is the solved sequence, `grad_controls` [H*I, n] is dL/d(controls).  Returns a dict of
        dL/d(input) of the input's shape, keyed "A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", plus
        "kkt_residual" [n] (max |gradient| over the free components); `want` names the outputs to compute.
        Instances with non-finite data or a model that breaks dlib's requires clause get zeros and raise last_flags
        (want_flags=False leaves last_flags at 0 and keeps a DEVICE call asynchronous)."""
        p = self._params(**over)
        H = p.horizon
        _check_names("gradient", want, self.GRAD_NAMES)
        ar, I = self._general(A, R, inputs)
        rows = _rows(I, H)
        out = {k: ar.new(rows[k]) for k in want}
        to = {"d" + k: ar.addr(a) for k, a in out.items() if k != "kkt_residual"}
        io = self._io(ar, I, H, (A, B, Cc, Q, R, lower, upper, x0, targets))
        g = capi.GeneralGrad(controls=ar.read(controls, H * I), grad_controls=ar.read(grad_controls, H * I),
                             kkt_residual=ar.addr(out.get("kkt_residual")), **to)
        self._run(self._lib.tpc_mpc_solve_batch_general_backward, p, ar, C.byref(io), C.byref(g), want_flags=want_flags)
        if "kkt_residual" in out:
            out["kkt_residual"] = out["kkt_residual"].reshape(ar.n)
        return out

    @staticmethod
    def _device_only(ar):
        if ar.mem != capi.DEVICE:
            raise ValueError("this entry takes CUDA tensors only")
        return ar

    @staticmethod
    def _plant(ar, plant, disturbance, I, steps, match="shape"):
        """capi.Plant of plant=(Ap, Bp, Cp) | None and disturbance [steps*2, n] | None"""
        if plant is not None and len(plant) != 3:
            raise ValueError("plant must be (Ap, Bp, Cp)")
        Ap, Bp, Cp = plant if plant is not None else (None, None, None)
        return capi.Plant(A=ar.read(Ap, 4, None, match), B=ar.read(Bp, 2 * I, None, match),
                          C=ar.read(Cp, 2, None, match), disturbance=ar.read(disturbance, 2 * steps, None, match),
                          ld_d=0 if disturbance is None else ar.n)

    def rollout(self, steps: int, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets=None,
                controls=None, v_state=None, inputs: Optional[int] = None, want_states: bool = True,
                want_iters: bool = False, **over):
        """`steps` successive operator() calls per controller with warm start and target shift
        (mpc.h:229-239) and the plant update of dlib/test/mpc.cpp:314 between them.  SoA arrays as
        in solve_batch_general; new_last_targets [2*steps, n].  Returns (controls[steps*I, n],
        states[steps*2, n] | None, iters[steps, n] | None)."""
        c_out, s_out, i_out, _ = self._rollout(False, steps, A, B, Cc, Q, R, lower, upper, x0, targets,
                                               new_last_targets, controls, v_state, inputs, want_states, want_iters,
                                               **over)
        return c_out, s_out, i_out

    def rollout_record(self, steps: int, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets=None,
                       controls=None, v_state=None, inputs: Optional[int] = None, want_iters: bool = False,
                       plant=None, disturbance=None, **over):
        """rollout that also records every step's solved sequence (tpc_mpc_rollout_record), what rollout_backward
        differentiates at.  Returns (controls[steps*I, n], states[steps*2, n], sequences[steps*H*I, n],
        iters[steps, n] | None); the first two and iters are rollout's, bit for bit.  plant=(Ap, Bp, Cp) and / or
        disturbance [steps*2, n] move the state instead of the controller's model (tpc_mpc_rollout_plant, fp64)."""
        c_out, s_out, i_out, q_out = self._rollout(True, steps, A, B, Cc, Q, R, lower, upper, x0, targets,
                                                   new_last_targets, controls, v_state, inputs, True, want_iters,
                                                   plant=plant, disturbance=disturbance, **over)
        return c_out, s_out, q_out, i_out

    def _rollout(self, record, steps, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets, controls, v_state,
                 inputs, want_states, want_iters, plant=None, disturbance=None, **over):
        p = self._params(**over)
        H = p.horizon
        ar, I = self._general(A, R, inputs, p.dtype)
        io = self._io(ar, I, H, (A, B, Cc, Q, R, lower, upper, x0, targets), controls, v_state)
        c_out = ar.new(steps * I)
        s_out = ar.new(steps * 2) if want_states else None
        i_out = ar.new(steps, dtype=_I32) if want_iters else None
        q_out = ar.new(steps * H * I) if record else None
        nlt = ar.read(new_last_targets, 2 * steps)
        outs = (ar.addr(c_out), ar.addr(s_out), ar.addr(i_out))
        if plant is not None or disturbance is not None:
            pl = self._plant(ar, plant, disturbance, I, steps)
            entry = self._lib.tpc_mpc_rollout_plant
            args = (C.byref(io), C.byref(pl), capi.LOOP_RECORD, int(steps), nlt, None, 0, *outs, ar.addr(q_out), None)
        elif record:
            entry, args = self._lib.tpc_mpc_rollout_record, (C.byref(io), int(steps), nlt, *outs, ar.addr(q_out))
        else:
            entry, args = self._lib.tpc_mpc_rollout, (C.byref(io), int(steps), nlt, *outs)
        self._run(entry, p, ar, *args)
        return c_out, s_out, i_out, q_out

    def rollout_polished(self, steps: int, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets=None,
                         controls=None, v_state=None, inputs: Optional[int] = None, tol: float = 1e-9,
                         max_rounds: int = 8, want_status: bool = True, want_iters: bool = False, residuals=None,
                         plant=None, disturbance=None, **over):
        """rollout with every step's solved sequence polished onto the verified optimum before the plant moves
        (tpc_mpc_rollout_polished: the solve of rollout's step, then polish_batch_general's rule and the step in one
        kernel), fp64 only.  Arrays as in rollout (numpy: HOST memory, CUDA torch tensors: DEVICE memory on the
        current stream).  Returns (controls[steps*I, n], states[steps*2, n], sequences[steps*H*I, n],
        status[steps, n] | None, iters[steps, n] | None): sequences are the polished ones -- what rollout_backward
        takes -- and status holds the polish rounds of each (step, instance), or -1 where the step kept the solver's
        sequence (last_flags then carries FLAG_NOT_POLISHED).  want_status=False returns None for status, leaves
        last_flags at 0 and keeps a DEVICE call asynchronous.  residuals: optionally a pair of fp64 arrays [steps, n]
        of the inputs' kind that receive the polish's residual_in and residual_out of every (step, instance).
        plant=(Ap, Bp, Cp) and / or disturbance [steps*2, n]: the state moves with x <- Ap x + Bp u0 + Cp + d_k
        instead of the controller's model (tpc_mpc_rollout_plant); both None is the existing entry."""
        return self._rollout_exact(None, steps, (A, B, Cc, Q, R, lower, upper, x0, targets), new_last_targets,
                                   controls=controls, v_state=v_state, inputs=inputs, tol=tol, max_rounds=max_rounds,
                                   want_status=want_status, want_iters=want_iters, residuals=residuals, plant=plant,
                                   disturbance=disturbance, **over)

    def rollout_newton(self, steps: int, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets=None,
                       controls=None, v_state=None, inputs: Optional[int] = None, tol: float = 1e-9,
                       max_rounds: int = 8, fallback: str = "solve", want_status: bool = True,
                       want_iters: bool = False, residuals=None, plant=None, disturbance=None, **over):
        """The polished closed loop with the Newton rounds first (tpc_mpc_rollout_newton), fp64 only: every step is
        polished from the shifted warm start without a first-order solve, all steps in one launch; an instance is
        carried as long as the polish verifies.  fallback="solve": the instances that stopped are run from step 0
        through rollout_polished's loop and written back; fallback="none": their rows from the stop on are status -1
        and zeros, and last_flags carries FLAG_NOT_POLISHED (the only mode of a host-only solver, device=None).
        Arguments and arrays as rollout_polished.  Returns rollout_polished's tuple plus first_unverified:
        (controls[steps*I, n], states[steps*2, n], sequences[steps*H*I, n], status[steps, n] | None,
        iters[steps, n] | None, first_unverified[n]) -- int32, the step phase 1 stopped at, `steps` for an instance
        it carried to the end.  iters is 0 for the steps of such an instance.  plant, disturbance: as
        rollout_polished."""
        return self._rollout_exact(fallback, steps, (A, B, Cc, Q, R, lower, upper, x0, targets), new_last_targets,
                                   controls=controls, v_state=v_state, inputs=inputs, tol=tol, max_rounds=max_rounds,
                                   want_status=want_status, want_iters=want_iters, residuals=residuals, plant=plant,
                                   disturbance=disturbance, **over)

    def _rollout_exact(self, newton, steps, model, new_last_targets, *, controls, v_state, inputs, tol, max_rounds,
                       want_status, want_iters, residuals, plant, disturbance, **over):
        """rollout_polished (newton=None) and rollout_newton (newton=its fallback): the same arrays, the Newton loop
        with `first_unverified` and the fallback on top."""
        p = self._params(**over)
        H = p.horizon
        ar, I = self._general(model[0], model[4], inputs)
        io = self._io(ar, I, H, model, controls, v_state)
        c_out, s_out, q_out = ar.new(steps * I), ar.new(steps * 2), ar.new(steps * H * I)
        i_out = ar.new(steps, dtype=_I32) if want_iters else None
        status = ar.new(steps, dtype=_I32) if want_status else None
        first = ar.new(1, dtype=_I32) if newton else None
        rin, rout = residuals if residuals is not None else (None, None)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=ar.addr(status),
                        residual_in=ar.update(rin, steps), residual_out=ar.update(rout, steps))
        nlt = ar.read(new_last_targets, 2 * steps)
        fb = capi.NEWTON_FALLBACKS[newton] if newton else 0
        outs = (ar.addr(c_out), ar.addr(s_out), ar.addr(i_out), ar.addr(q_out))
        if plant is not None or disturbance is not None:   # the same loop against a separate plant
            pl = self._plant(ar, plant, disturbance, I, steps)
            entry = self._lib.tpc_mpc_rollout_plant
            args = (C.byref(io), C.byref(pl), capi.LOOP_NEWTON if newton else capi.LOOP_POLISHED, int(steps), nlt,
                    C.byref(q), fb, *outs, ar.addr(first))
        elif newton:
            entry = self._lib.tpc_mpc_rollout_newton
            args = (C.byref(io), int(steps), nlt, C.byref(q), fb, *outs, ar.addr(first))
        else:
            entry, args = self._lib.tpc_mpc_rollout_polished, (C.byref(io), int(steps), nlt, C.byref(q), *outs)
        self._run(entry, p, ar, *args, want_flags=want_status)
        out = (c_out, s_out, q_out, status, i_out)
        return out + (first[0],) if newton else out

    def rollout_compact_exact(self, steps: int, v, delta_y, delta_phi, x0=None, tol: float = 1e-9,
                              max_rounds: int = 16, fallback: str = "solve", want_states: bool = True,
                              want_sequences: bool = True, want_status: bool = True, residuals=None, **over):
        """The reference controller rolled forward `steps` steps on its own model, every step the verified optimum
        (tpc_mpc_rollout_compact_exact), fp64 only: rollout_newton on the model solve_batch_compact_exact builds from
        (v, delta_y, delta_phi) -- the target stays (delta_y, delta_phi) at every step -- without the general form:
        three vectors [n] in (and x0 [2, n], None = zeros), all steps of an instance in one lane, one launch.
        fallback="solve": the instances the Newton rounds stopped are expanded on the device, run from step 0 through
        rollout_polished's loop and written back; fallback="none": their rows from the stop on are status -1 and zeros
        and last_flags carries FLAG_NOT_POLISHED (the only mode of a host-only solver, device=None).  Arrays as in
        solve_batch_compact_exact (numpy: HOST memory, CUDA tensors: DEVICE memory on the current stream).  Returns
        (controls[steps*2, n], states[steps*2, n] | None, sequences[steps*H*2, n] | None, status[steps, n] | None,
        first_unverified[n] | None): rollout_newton's rows on the expanded arrays, bit for bit for an instance carried
        to the end; status holds the Newton rounds of each (step, instance) and first_unverified (int32) the step
        phase 1 stopped at, `steps` for an instance it carried through -- both None with want_status=False, which with
        fallback="none" also leaves last_flags at 0 and keeps a DEVICE call asynchronous.  residuals: optionally a pair
        of fp64 arrays [steps, n] of the inputs' kind that receive residual_in and residual_out of every (step,
        instance).  sequences and states are what rollout_compact_exact_backward takes, and rollout_backward on the
        expanded arrays (autograd: mpc_rollout_compact)."""
        p = self._params(**over)
        H, S = p.horizon, int(steps)
        ar = Arrays(v)
        vectors = ar.read_rows((v, delta_y, delta_phi), None, "length")
        c_out = ar.new(S * 2)
        s_out = ar.new(S * 2) if want_states else None
        q_out = ar.new(S * H * 2) if want_sequences else None
        status = ar.new(S, dtype=_I32) if want_status else None
        first = ar.new(dtype=_I32) if want_status else None
        rin, rout = residuals if residuals is not None else (None, None)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=ar.addr(status),
                        residual_in=ar.update(rin, S), residual_out=ar.update(rout, S))
        self._run(self._lib.tpc_mpc_rollout_compact_exact, p, ar, ar.n, *vectors, ar.read(x0, 2), S, C.byref(q),
                  capi.NEWTON_FALLBACKS[fallback], ar.addr(c_out), ar.addr(s_out), ar.addr(q_out), ar.addr(first),
                  want_flags=want_status or fallback != "none")
        return c_out, s_out, q_out, status, first

    COMPACT_LOOP_GRAD_NAMES = ("v", "delta_y", "delta_phi", "x0", "params", "params_rows", "kkt_residual")

    def rollout_compact_exact_backward(self, steps: int, v, delta_y, delta_phi, x0=None, *, sequences, states,
                                       status=None, grad_controls=None, grad_states=None,
                                       want=("v", "delta_y", "delta_phi", "x0", "params"), want_flags: bool = True,
                                       **over):
        """Backward pass of rollout_compact_exact (tpc_mpc_rollout_compact_exact_backward), fp64 only: the gradient
        of a loss of the loop's controls and states, taken at what rollout_compact_exact returned (`sequences`
        [steps*H*2, n], `states` [steps*2, n]) -- one launch over all steps, no general form.

        Arrays as in rollout_compact_exact (numpy: HOST memory, CUDA tensors: DEVICE memory on the current stream):
        v, delta_y, delta_phi [n], x0 [2, n] or None (zeros), `status` (int32 [steps, n], optional: an instance with a
        negative status at any step is excluded).  grad_controls / grad_states [steps*2, n] are dL/d(controls) /
        dL/d(states) (None: zero).  Returns a dict keyed by `want`: "v", "delta_y", "delta_phi" [n], "x0" [2, n] (also
        without an x0: the gradient at the zero start), "params" [10] (the gradient of the shared parameters in the
        order of COMPACT_PARAM_NAMES, summed over the batch on the device in a fixed order, the same bytes on every
        call), "params_rows" [10, n] (per instance) and "kkt_residual" [n] (max over the steps).  Excluded instances
        (negative status, non-finite data: last_flags) get zeros and add nothing to "params"; want_flags=False leaves
        last_flags at 0 and keeps a DEVICE call asynchronous."""
        p = self._params(**over)
        H, S = p.horizon, int(steps)
        _check_names("gradient", want, self.COMPACT_LOOP_GRAD_NAMES)
        ar = Arrays(v)
        NP = len(COMPACT_PARAM_NAMES)
        rows = {"params_rows": NP, "x0": 2}
        out = {k: ar.new(NP, per_instance=False) if k == "params" else ar.new(rows[k]) if k in rows else ar.new()
               for k in self.COMPACT_LOOP_GRAD_NAMES if k in want}
        to = {k: ar.addr(a) for k, a in out.items()}
        g = capi.CompactLoopGrad(grad_controls=ar.read(grad_controls, S * 2), grad_states=ar.read(grad_states, S * 2),
                                 dv=to.get("v"), ddelta_y=to.get("delta_y"), ddelta_phi=to.get("delta_phi"),
                                 dx0=to.get("x0"), dparams_rows=to.get("params_rows"), dparams=to.get("params"),
                                 kkt_residual=to.get("kkt_residual"))
        self._run(self._lib.tpc_mpc_rollout_compact_exact_backward, p, ar, ar.n, ar.read(v), ar.read(delta_y),
                  ar.read(delta_phi), ar.read(x0, 2), S, ar.read(sequences, S * H * 2), ar.read(states, S * 2),
                  ar.read(status, S, dtype=_I32), C.byref(g), want_flags=want_flags)
        return out

    ROLLOUT_GRAD_NAMES = GRAD_NAMES[:-1] + ("new_last_targets", "kkt_residual")
    PLANT_GRAD_NAMES = ("Ap", "Bp", "Cp", "disturbance")

    def rollout_backward(self, steps: int, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets=None, *,
                         sequences, states, grad_controls=None, grad_states=None, inputs: Optional[int] = None,
                         want=None, want_flags: bool = True, plant=None, disturbance=None, **over):
        """Backward pass of rollout (tpc_mpc_rollout_backward), fp64 only: the gradient of a loss of the rollout's
        controls and states, taken at what rollout_record returned (`sequences` [steps*H*I, n], `states`
        [steps*2, n]).  grad_controls [steps*I, n] / grad_states [steps*2, n] are dL/d(controls) / dL/d(states)
        (None: zero).  Arrays as in rollout (numpy: HOST memory, CUDA torch tensors: DEVICE memory on the current
        stream).  Returns a dict keyed "A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets",
        "new_last_targets" (only when new_last_targets is given) and "kkt_residual" [n] (max over the steps); `want`
        names the outputs to compute.  Flagged instances get zeros (last_flags; want_flags=False leaves it at 0 and
        keeps a DEVICE call asynchronous).  With plant=(Ap, Bp, Cp) (tpc_mpc_rollout_plant_backward) the keys "Ap",
        "Bp", "Cp" hold the plant's gradients and "A", "B", "C" the controller's alone; "disturbance" [steps*2, n] is
        the gradient of the disturbance's rows (at zero when disturbance is None) and has to be named in `want`
        unless a plant or a disturbance is given."""
        p = self._params(**over)
        H = p.horizon
        plant_call = plant is not None or disturbance is not None
        if want is None:
            want = tuple(k for k in self.ROLLOUT_GRAD_NAMES if k != "new_last_targets" or new_last_targets is not None)
            if plant is not None:
                want += ("Ap", "Bp", "Cp")
            if plant_call:
                want += ("disturbance",)
        plant_call = plant_call or bool(set(want) & set(self.PLANT_GRAD_NAMES))
        _check_names("gradient", want, self.ROLLOUT_GRAD_NAMES + self.PLANT_GRAD_NAMES)
        ar, I = self._general(A, R, inputs)
        rows = _rows(I, H, steps)
        out = {k: ar.new(rows[k]) for k in want}
        to = {k: ar.addr(a) for k, a in out.items()}
        io = self._io(ar, I, H, (A, B, Cc, Q, R, lower, upper, x0, targets))
        g = capi.RolloutGrad(sequences=ar.read(sequences, steps * H * I), states=ar.read(states, 2 * steps),
                             grad_controls=ar.read(grad_controls, steps * I), grad_states=ar.read(grad_states, 2 * steps),
                             dnew_last_targets=to.get("new_last_targets"), kkt_residual=to.get("kkt_residual"),
                             **{"d" + k: to.get(k) for k in self.GRAD_NAMES[:-1]})
        nlt = ar.read(new_last_targets, 2 * steps)
        if plant_call:
            pl = self._plant(ar, plant, None, I, steps)   # (the disturbance itself is not read: the states are recorded)
            pg = capi.PlantGrad(dA=to.get("Ap"), dB=to.get("Bp"), dC=to.get("Cp"), ddisturbance=to.get("disturbance"))
            entry = self._lib.tpc_mpc_rollout_plant_backward
            args = (C.byref(io), C.byref(pl), int(steps), nlt, C.byref(g), C.byref(pg))
        else:
            entry, args = self._lib.tpc_mpc_rollout_backward, (C.byref(io), int(steps), nlt, C.byref(g))
        self._run(entry, p, ar, *args, want_flags=want_flags)
        if "kkt_residual" in out:
            out["kkt_residual"] = out["kkt_residual"].reshape(ar.n)
        return out

    TANGENT_NAMES = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "new_last_targets")
    PLANT_TANGENT_NAMES = ("Ap", "Bp", "Cp", "disturbance")

    def _tangents(self, ar, rows, tangents):
        """(K, capi.Tangents, capi.PlantTangents) of `tangents`: names of TANGENT_NAMES and PLANT_TANGENT_NAMES ->
        arrays [K, c, n] (2-D [c, n]: K = 1) with c = rows[name]"""
        _check_names("tangent", tangents, self.TANGENT_NAMES + self.PLANT_TANGENT_NAMES)
        tangents = {k: v for k, v in tangents.items() if v is not None}
        if not tangents:
            raise ValueError("tangents is empty: give at least one direction array")
        K = _directions(tangents, lambda name: 3, "[K, c, n] (or [c, n] for K = 1)")
        at = {name: ar.read(v, K * rows[name], None, "loose") for name, v in tangents.items()}
        tan = capi.Tangents(directions=K, reserved=0, **{"t" + name: at.get(name) for name in self.TANGENT_NAMES})
        ptan = capi.PlantTangents(tA=at.get("Ap"), tB=at.get("Bp"), tC=at.get("Cp"), tdisturbance=at.get("disturbance"))
        return K, tan, ptan

    def solve_batch_general_forward(self, A, B, Cc, Q, R, lower, upper, x0, targets, controls, tangents,
                                    inputs: Optional[int] = None, want_flags: bool = True, **over):
        """Forward mode of solve_batch_general (tpc_mpc_solve_batch_general_forward), fp64 only: the directional
        derivatives of the controls along K directions, taken at `controls` [H*I, n].  `tangents` maps the names "A",
        "B", "C", "Q", "R", "lower", "upper", "x0", "targets" to arrays [K, c, n] (c the rows of that input; a 2-D
        [c, n] array means K = 1; a missing name is a zero tangent).  Arrays as in solve_batch_general_backward (numpy:
        HOST memory, CUDA torch tensors: DEVICE memory on the current stream).  Returns tcontrols [K, H*I, n]; a
        flagged (direction, instance) pair gets zeros (last_flags)."""
        p = self._params(**over)
        H = p.horizon
        if set(tangents) & ({"new_last_targets"} | set(self.PLANT_TANGENT_NAMES)):
            raise ValueError("the single solve has no new_last_targets and no plant")
        ar, I = self._general(A, R, inputs)
        K, tan, _ = self._tangents(ar, _rows(I, H), tangents)
        io = self._io(ar, I, H, (A, B, Cc, Q, R, lower, upper, x0, targets), match="loose")
        tu = ar.new(K, H * I)
        self._run(self._lib.tpc_mpc_solve_batch_general_forward, p, ar, C.byref(io),
                  ar.read(controls, H * I, None, "loose"), C.byref(tan), ar.addr(tu), want_flags=want_flags)
        return tu

    def rollout_forward(self, steps: int, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets=None, *,
                        sequences, states, tangents, inputs: Optional[int] = None, want_states: bool = True,
                        want_flags: bool = True, plant=None, disturbance=None, **over):
        """Forward mode of rollout (tpc_mpc_rollout_forward), fp64 only: the directional derivatives of the rollout's
        controls and states along K directions, taken at what rollout_record / rollout_polished / rollout_newton
        returned (`sequences` [steps*H*I, n], `states` [steps*2, n]); all K directions and all steps run in one
        launch.  `tangents`: as in solve_batch_general_forward, plus "new_last_targets" [K, steps*2, n] (only with
        new_last_targets).  Returns (tcontrols [K, steps*I, n], tstates [K, steps*2, n] | None); a flagged (direction,
        instance) pair gets zeros (last_flags; want_flags=False keeps a DEVICE call asynchronous).  With
        plant=(Ap, Bp, Cp) (tpc_mpc_rollout_plant_forward) `tangents` may hold "Ap", "Bp", "Cp" and the tangents "A",
        "B", "C" enter the steps' QPs only; "disturbance" [K, steps*2, n] is the tangent of the disturbance's rows."""
        p = self._params(**over)
        H = p.horizon
        plant_call = plant is not None or disturbance is not None or bool(set(tangents) & set(self.PLANT_TANGENT_NAMES))
        ar, I = self._general(A, R, inputs)
        K, tan, ptan = self._tangents(ar, _rows(I, H, steps), tangents)
        io = self._io(ar, I, H, (A, B, Cc, Q, R, lower, upper, x0, targets), match="loose")
        tu = ar.new(K, steps * I)
        tx = ar.new(K, steps * 2) if want_states else None
        at = (ar.read(new_last_targets, 2 * steps, None, "loose"), ar.read(sequences, steps * H * I, None, "loose"),
              ar.read(states, 2 * steps, None, "loose"), C.byref(tan))
        if plant_call:
            pl = self._plant(ar, plant, None, I, steps, "loose")   # (the disturbance itself is not read: the states are recorded)
            entry = self._lib.tpc_mpc_rollout_plant_forward
            args = (C.byref(io), C.byref(pl), int(steps), *at, C.byref(ptan))
        else:
            entry, args = self._lib.tpc_mpc_rollout_forward, (C.byref(io), int(steps), *at)
        self._run(entry, p, ar, *args, ar.addr(tu), ar.addr(tx), want_flags=want_flags)
        return tu, tx

    def follow_batch(self, pos_x, pos_y, dir_x, dir_y, velocity, count, car_velocity, look_ahead,
                     lookup=None, want_iters: bool = False, **over):
        """Batched tobiMPC branch of cycle() on raw trajectories (device tensors).

        pos_x .. velocity: float32 CUDA tensors [max_points, n] (point-major, SoA); count int32 [n];
        car_velocity, look_ahead float32 [n]; lookup: optional (x, y) float32 CUDA tensors of the
        velocity lookup table.  Returns (steering_front f64, steering_rear f64, target_speed f32,
        target_distance f32[, iters])."""
        return self._follow(False, pos_x, pos_y, dir_x, dir_y, velocity, count, car_velocity, look_ahead,
                            step_spacing=None, lookup=lookup, want_iters=want_iters, want_targets=False, **over)

    def follow_batch_horizon(self, pos_x, pos_y, dir_x, dir_y, velocity, count, car_velocity, look_ahead,
                             step_spacing=None, lookup=None, want_iters: bool = False,
                             want_targets: bool = False, **over):
        """follow_batch with one trajectory point per horizon step (tpc_mpc_follow_batch_horizon):
        step t's target is the polyline point at arc length look_ahead + t * spacing.  step_spacing:
        optional float32 CUDA tensor [n] (None: |v| * step_size).  Returns (front, rear, target_speed,
        target_distance[, targets f64 [2H, n]][, iters])."""
        return self._follow(True, pos_x, pos_y, dir_x, dir_y, velocity, count, car_velocity, look_ahead,
                            step_spacing=step_spacing, lookup=lookup, want_iters=want_iters, want_targets=want_targets,
                            **over)

    def _follow(self, horizon, pos_x, pos_y, dir_x, dir_y, velocity, count, car_velocity, look_ahead, *, step_spacing,
                lookup, want_iters, want_targets, **over):
        """follow_batch (tpc_mpc_follow_batch) and, with horizon=True, follow_batch_horizon with its two options"""
        p = self._params(**over)
        P, n = pos_x.shape
        ar = self._device_only(Arrays(pos_x, n, np.float32))
        tr = capi.Trajectories(n=n, ld=n, max_points=P, pos_x=ar.read(pos_x, P), pos_y=ar.read(pos_y, P),
                               dir_x=ar.read(dir_x, P), dir_y=ar.read(dir_y, P), velocity=ar.read(velocity, P),
                               count=ar.read(count, None, _I32, "length"),
                               car_velocity=ar.read(car_velocity, match="length"),
                               look_ahead=ar.read(look_ahead, match="length"))
        front, rear = ar.new(dtype=np.float64), ar.new(dtype=np.float64)
        tspeed, tdist = ar.new(), ar.new()
        targets = ar.new(2 * p.horizon, dtype=np.float64) if want_targets else None
        iters = ar.new(dtype=_I32) if want_iters else None
        lx, ly, ln = (None, None, 0) if lookup is None else (lookup[0].data_ptr(), lookup[1].data_ptr(), lookup[0].numel())
        outs = (ar.addr(front), ar.addr(rear), ar.addr(tspeed), ar.addr(tdist))
        if horizon:
            self._run(self._lib.tpc_mpc_follow_batch_horizon, p, ar, C.byref(tr), ar.read(step_spacing, match="length"),
                      lx, ly, ln, *outs, ar.addr(targets), ar.addr(iters), mem=False)
        else:
            self._run(self._lib.tpc_mpc_follow_batch, p, ar, C.byref(tr), lx, ly, ln, *outs, ar.addr(iters), mem=False)
        out = (front, rear, tspeed, tdist) + ((targets,) if want_targets else ())
        return out + (iters,) if want_iters else out
