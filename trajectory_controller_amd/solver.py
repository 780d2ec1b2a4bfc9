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

_NP = {capi.F64: np.float64, capi.F32: np.float32}
COMPACT_PARAM_NAMES = capi.COMPACT_PARAM_NAMES   # the order of solve_batch_compact_exact_backward's "params"


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


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
        elif _is_torch(hint):
            import torch
            if not (hint.is_cuda and hint.dtype == torch.int32 and hint.is_contiguous()):
                raise ValueError("a device hint must be a contiguous int32 CUDA tensor")
            self._hint_ref = hint
            self._check(self._lib.tpc_mpc_x_set_work_hint(self._h, hint.data_ptr(), hint.numel(), capi.DEVICE))
        else:
            h = np.ascontiguousarray(hint, dtype=np.int32)
            self._check(self._lib.tpc_mpc_x_set_work_hint(self._h, h.ctypes.data, h.shape[0], capi.HOST))

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
        if _is_torch(v):
            import torch
            tdt = torch.float64 if p.dtype == capi.F64 else torch.float32
            n = v.numel()
            for t in (v, delta_y, delta_phi):
                if not (t.is_cuda and t.dtype == tdt and t.is_contiguous() and t.numel() == n):
                    raise ValueError("device batch arrays must be contiguous CUDA tensors of the solver dtype")
            if out is None:
                front, rear = torch.empty_like(v), torch.empty_like(v)
            else:
                front, rear = out
            iters = torch.empty(n, dtype=torch.int32, device=v.device) if want_iters else None
            flags = C.c_uint32(0)
            stream = torch.cuda.current_stream(v.device).cuda_stream
            self._check(self._lib.tpc_mpc_solve_batch_compact(
                self._h, C.byref(p), n, v.data_ptr(), delta_y.data_ptr(), delta_phi.data_ptr(),
                front.data_ptr(), rear.data_ptr(), iters.data_ptr() if want_iters else None,
                C.byref(flags) if want_flags else None, capi.DEVICE, C.c_void_p(stream)))
            self.last_flags = flags.value
        else:
            dt = _NP[p.dtype]
            v, delta_y, delta_phi = (np.ascontiguousarray(a, dtype=dt) for a in (v, delta_y, delta_phi))
            n = v.shape[0]
            front, rear = np.empty(n, dtype=dt), np.empty(n, dtype=dt)
            iters = np.empty(n, dtype=np.int32) if want_iters else None
            flags = C.c_uint32(0)
            self._check(self._lib.tpc_mpc_solve_batch_compact(
                self._h, C.byref(p), n, v.ctypes.data, delta_y.ctypes.data, delta_phi.ctypes.data,
                front.ctypes.data, rear.ctypes.data, iters.ctypes.data if want_iters else None,
                C.byref(flags), capi.HOST, None))
            self.last_flags = flags.value
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
        fb = capi.NEWTON_FALLBACKS[fallback]
        rows_shape = (len(COMPACT_PARAM_NAMES), v.numel() if _is_torch(v) else np.shape(v)[0])
        if _is_torch(v):
            import torch
            n = v.numel()
            for t in (v, delta_y, delta_phi):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n):
                    raise ValueError("device batch arrays must be contiguous fp64 CUDA tensors")
            if params_rows is not None and not (
                    _is_torch(params_rows) and params_rows.is_cuda and params_rows.dtype == torch.float64
                    and params_rows.is_contiguous() and tuple(params_rows.shape) == rows_shape):
                raise ValueError(f"params_rows must be a contiguous fp64 CUDA tensor {list(rows_shape)}")
            if start is not None and not (
                    _is_torch(start) and start.is_cuda and start.dtype == torch.float64 and start.is_contiguous()
                    and tuple(start.shape) == (2 * H, n)):
                raise ValueError(f"start must be a contiguous fp64 CUDA tensor {[2 * H, n]}")

            def new(dtype, rows=None):
                t = torch.empty(n if rows is None else (rows, n),
                                dtype=torch.float64 if dtype is np.float64 else torch.int32, device=v.device)
                return t, t.data_ptr()
            ptr = lambda t: t.data_ptr()
            stream = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
            mem = capi.DEVICE
        else:
            v, delta_y, delta_phi = (np.ascontiguousarray(a, dtype=np.float64) for a in (v, delta_y, delta_phi))
            n = v.shape[0]
            if params_rows is not None:
                params_rows = np.ascontiguousarray(params_rows, dtype=np.float64)
                if params_rows.shape != rows_shape:
                    raise ValueError(f"params_rows must be an array {list(rows_shape)}")
            if start is not None:
                start = np.ascontiguousarray(start, dtype=np.float64)
                if start.shape != (2 * H, n):
                    raise ValueError(f"start must be an array {[2 * H, n]}")

            def new(dtype, rows=None):
                a = np.empty(n if rows is None else (rows, n), dtype=dtype)
                return a, a.ctypes.data
            ptr = lambda a: a.ctypes.data
            stream = None
            mem = capi.HOST
        front, fp = new(np.float64)
        rear, rp = new(np.float64)
        seq, sqp = new(np.float64, 2 * H) if want_sequence else (None, None)
        status, sp = new(np.int32) if want_status else (None, None)
        fell, fbp = new(np.int32) if want_status and fallback != "none" else (None, None)
        rin, rip = new(np.float64) if want_residuals else (None, None)
        rout, rop = new(np.float64) if want_residuals else (None, None)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=sp, residual_in=rip,
                        residual_out=rop)
        flags = C.c_uint32(0)
        fp_flags = C.byref(flags) if want_status or fallback != "none" else None
        if start is not None:
            self._check(self._lib.tpc_mpc_solve_batch_compact_exact_from(
                self._h, C.byref(p), n, ptr(v), ptr(delta_y), ptr(delta_phi),
                None if params_rows is None else ptr(params_rows), ptr(start), C.byref(q), fb, fp, rp, sqp, fbp,
                fp_flags, mem, stream))
        elif params_rows is None:
            self._check(self._lib.tpc_mpc_solve_batch_compact_exact(
                self._h, C.byref(p), n, ptr(v), ptr(delta_y), ptr(delta_phi), C.byref(q), fb, fp, rp, sqp, fbp,
                fp_flags, mem, stream))
        else:
            self._check(self._lib.tpc_mpc_solve_batch_compact_exact_rows(
                self._h, C.byref(p), n, ptr(v), ptr(delta_y), ptr(delta_phi), ptr(params_rows), C.byref(q), fb, fp,
                rp, sqp, fbp, fp_flags, mem, stream))
        self.last_flags = flags.value
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
        unknown = set(want) - set(self.COMPACT_GRAD_NAMES)
        if unknown:
            raise ValueError(f"unknown gradient names {sorted(unknown)}")
        if _is_torch(v):
            import torch
            n = v.numel()

            def ptr(t, rows=None, dtype=torch.float64):
                if t is None:
                    return None
                shape = (n,) if rows is None else (rows, n)
                if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"expected a contiguous {dtype} CUDA tensor {list(shape)}")
                return t.data_ptr()

            def new(shape):
                t = torch.empty(shape, dtype=torch.float64, device=v.device)
                return t, t.data_ptr()
            i32 = torch.int32
            stream = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
            mem = capi.DEVICE
        else:
            v = np.ascontiguousarray(v, dtype=np.float64)
            n = v.shape[0]
            keep = []

            def ptr(a, rows=None, dtype=np.float64):
                if a is None:
                    return None
                a = np.ascontiguousarray(a, dtype=dtype)
                if a.shape != ((n,) if rows is None else (rows, n)):
                    raise ValueError(f"expected an array {[n] if rows is None else [rows, n]}")
                keep.append(a)
                return a.ctypes.data

            def new(shape):
                a = np.empty(shape, dtype=np.float64)
                return a, a.ctypes.data
            i32 = np.int32
            stream = None
            mem = capi.HOST
        shapes = {"v": n, "delta_y": n, "delta_phi": n, "params": len(COMPACT_PARAM_NAMES),
                  "params_rows": (len(COMPACT_PARAM_NAMES), n), "kkt_residual": n}
        out, optr = {}, {}
        for k in self.COMPACT_GRAD_NAMES:
            out[k], optr[k] = new(shapes[k]) if k in want else (None, None)
        g = capi.CompactGrad(grad_front=ptr(grad_front), grad_rear=ptr(grad_rear),
                             grad_sequence=ptr(grad_sequence, 2 * H), dv=optr["v"], ddelta_y=optr["delta_y"],
                             ddelta_phi=optr["delta_phi"], dparams_rows=optr["params_rows"], dparams=optr["params"],
                             kkt_residual=optr["kkt_residual"])
        flags = C.c_uint32(0)
        if params_rows is None:
            self._check(self._lib.tpc_mpc_solve_batch_compact_exact_backward(
                self._h, C.byref(p), n, ptr(v), ptr(delta_y), ptr(delta_phi), ptr(sequence, 2 * H),
                ptr(status, dtype=i32), C.byref(g), C.byref(flags) if want_flags else None, mem, stream))
        else:
            self._check(self._lib.tpc_mpc_solve_batch_compact_exact_rows_backward(
                self._h, C.byref(p), n, ptr(v), ptr(delta_y), ptr(delta_phi),
                ptr(params_rows, len(COMPACT_PARAM_NAMES)), ptr(sequence, 2 * H), ptr(status, dtype=i32), C.byref(g),
                C.byref(flags) if want_flags else None, mem, stream))
        self.last_flags = flags.value
        return {k: a for k, a in out.items() if a is not None}

    def solve_batch_compact_mixed(self, horizons, v, delta_y, delta_phi, want_iters: bool = False, **over):
        """Mixed-horizon batch (BASELINE config 5): instance k is solved with horizon horizons[k]
        (tpc_mpc_solve_batch_compact_mixed: binned by horizon on the device, one launch sequence per
        bin, results back in the caller's order).  Arrays as in solve_batch_compact; `horizons` is an
        integer array/tensor of the same length."""
        p = self._params(**over)
        flags = C.c_uint32(0)
        if _is_torch(v):
            import torch
            tdt = torch.float64 if p.dtype == capi.F64 else torch.float32
            n = v.numel()
            for t in (v, delta_y, delta_phi):
                if not (t.is_cuda and t.dtype == tdt and t.is_contiguous() and t.numel() == n):
                    raise ValueError("device batch arrays must be contiguous CUDA tensors of the solver dtype")
            hz = torch.as_tensor(horizons, device=v.device).to(torch.int32).contiguous()
            if hz.numel() != n:
                raise ValueError("horizons must have one entry per instance")
            front, rear = torch.empty_like(v), torch.empty_like(v)
            iters = torch.empty(n, dtype=torch.int32, device=v.device) if want_iters else None
            stream = torch.cuda.current_stream(v.device).cuda_stream
            self._check(self._lib.tpc_mpc_solve_batch_compact_mixed(
                self._h, C.byref(p), n, hz.data_ptr(), v.data_ptr(), delta_y.data_ptr(), delta_phi.data_ptr(),
                front.data_ptr(), rear.data_ptr(), iters.data_ptr() if want_iters else None,
                C.byref(flags), capi.DEVICE, C.c_void_p(stream)))
        else:
            dt = _NP[p.dtype]
            v, delta_y, delta_phi = (np.ascontiguousarray(a, dtype=dt) for a in (v, delta_y, delta_phi))
            n = v.shape[0]
            hz = np.ascontiguousarray(horizons, dtype=np.int32)
            if hz.shape[0] != n:
                raise ValueError("horizons must have one entry per instance")
            front, rear = np.empty(n, dtype=dt), np.empty(n, dtype=dt)
            iters = np.empty(n, dtype=np.int32) if want_iters else None
            self._check(self._lib.tpc_mpc_solve_batch_compact_mixed(
                self._h, C.byref(p), n, hz.ctypes.data, v.ctypes.data, delta_y.ctypes.data, delta_phi.ctypes.data,
                front.ctypes.data, rear.ctypes.data, iters.ctypes.data if want_iters else None,
                C.byref(flags), capi.HOST, None))
        self.last_flags = flags.value
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
        import torch
        p = self._params(**over)
        tdt = torch.float64 if p.dtype == capi.F64 else torch.float32
        first, count, stride = C.c_int64(), C.c_int64(), C.c_int64()
        self._lib.tpc_mpc_shard_map(int(n_total), self.rank, self.world, capi.SPLITS[split], C.byref(first), C.byref(count),
                                    C.byref(stride))
        for t in (v_shard, dy_shard, dphi_shard):
            if not (t.is_cuda and t.dtype == tdt and t.is_contiguous() and t.numel() == count.value):
                raise ValueError(f"shard arrays must be contiguous CUDA tensors of the solver dtype holding this "
                                 f"rank's {count.value} instances (rank {self.rank} of {self.world}, n_total {n_total})")
        if out is None:
            front = torch.empty(n_total, dtype=tdt, device=v_shard.device)
            rear = torch.empty(n_total, dtype=tdt, device=v_shard.device)
        else:
            front, rear = out
        iters = torch.empty(v_shard.numel(), dtype=torch.int32, device=v_shard.device) if want_iters else None
        flags = C.c_uint32(0)
        stream = torch.cuda.current_stream(v_shard.device).cuda_stream
        self._check(self._lib.tpc_mpc_solve_batch_compact_sharded_split(
            self._h, C.byref(p), int(n_total), capi.SPLITS[split], v_shard.data_ptr(), dy_shard.data_ptr(), dphi_shard.data_ptr(),
            front.data_ptr(), rear.data_ptr(), iters.data_ptr() if want_iters else None,
            C.byref(flags) if want_flags else None, C.c_void_p(stream)))
        self.last_flags = flags.value
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
        import torch
        p = self._params(**over)
        H = p.horizon
        tdt = torch.float64 if p.dtype == capi.F64 else torch.float32
        n = A.shape[-1]
        I = inputs or R.shape[0]

        def ptr(t, rows):
            if not (t.is_cuda and t.dtype == tdt and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                raise ValueError(f"expected contiguous CUDA tensor [{rows},{n}] of the solver dtype")
            return t.data_ptr()
        u0 = torch.empty((I, n), dtype=tdt, device=A.device)
        iters = torch.zeros(n, dtype=torch.int32, device=A.device) if want_iters else None
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=None, v_inout=None, u0=u0.data_ptr(),
                            iters=iters.data_ptr() if want_iters else None)
        flags = C.c_uint32(0)
        stream = torch.cuda.current_stream(A.device).cuda_stream
        self._check(self._lib.tpc_mpc_solve_batch_general_sharded(self._h, C.byref(p), C.byref(io), C.byref(flags),
                                                                  C.c_void_p(stream)))
        self.last_flags = flags.value
        return (u0, iters) if want_iters else u0

    def solve_batch_general(self, A, B, Cc, Q, R, lower, upper, x0, targets, controls=None,
                            v_state=None, inputs: Optional[int] = None, want_iters: bool = False,
                            **over):
        """n independent dlib::mpc<2,I,H> controllers: ctor + set_target(t) + operator()(x0).

        Arrays are component-major (SoA): A[4,n] B[2I,n] C[2,n] Q[2,n] R[I,n] lower[I,n] upper[I,n]
        x0[2,n] targets[2H,n]; controls / v_state [H*I, n] are updated in place when given.
        Returns (u0[I,n][, iters])."""
        p = self._params(**over)
        H = p.horizon
        torch_mode = _is_torch(A)
        if torch_mode:
            import torch
            tdt = torch.float64 if p.dtype == capi.F64 else torch.float32
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, rows):
                if t is None:
                    return None
                if not (t.is_cuda and t.dtype == tdt and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                    raise ValueError(f"expected contiguous CUDA tensor [{rows},{n}] of the solver dtype")
                return t.data_ptr()
            u0 = torch.empty((I, n), dtype=tdt, device=A.device)
            iters = torch.empty(n, dtype=torch.int32, device=A.device) if want_iters else None
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
            ip = iters.data_ptr() if want_iters else None
            up = u0.data_ptr()
        else:
            dt = _NP[p.dtype]
            A = np.ascontiguousarray(A, dtype=dt)
            n = A.shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, rows):
                if a is None:
                    return None
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.shape == (rows, n)):
                    raise ValueError(f"expected C-contiguous ndarray [{rows},{n}] of the solver dtype")
                keep.append(a)
                return a.ctypes.data
            B, Cc, Q, R, lower, upper, x0, targets = (np.ascontiguousarray(a, dtype=dt) for a in
                                                      (B, Cc, Q, R, lower, upper, x0, targets))
            u0 = np.empty((I, n), dtype=dt)
            iters = np.empty(n, dtype=np.int32) if want_iters else None
            stream = None
            mem = capi.HOST
            ip = iters.ctypes.data if want_iters else None
            up = u0.ctypes.data
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=ptr(controls, H * I),
                            v_inout=ptr(v_state, H * I), u0=up, iters=ip)
        flags = C.c_uint32(0)
        self._check(self._lib.tpc_mpc_solve_batch_general(self._h, C.byref(p), C.byref(io),
                                                          C.byref(flags), mem, stream))
        self.last_flags = flags.value
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
        H = p.horizon
        if _is_torch(A):
            import torch
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, rows):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                    raise ValueError(f"expected contiguous fp64 CUDA tensor [{rows},{n}]")
                return t.data_ptr()

            def new(dtype):
                t = torch.empty(n, dtype=torch.float64 if dtype is np.float64 else torch.int32, device=A.device)
                return t, t.data_ptr()
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
        else:
            n = np.asarray(A).shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, rows):
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (rows, n):
                    raise ValueError(f"expected an array [{rows},{n}]")
                keep.append(a)
                return a.ctypes.data

            def new(dtype):
                a = np.empty(n, dtype=dtype)
                return a, a.ctypes.data
            if not (isinstance(controls, np.ndarray) and controls.dtype == np.float64 and controls.flags.c_contiguous):
                raise ValueError("controls must be a C-contiguous fp64 ndarray (it is updated in place)")
            stream = None
            mem = capi.HOST
        status, sp = new(np.int32) if want_status else (None, None)
        rin, rip = new(np.float64) if want_status else (None, None)
        rout, rop = new(np.float64) if want_status else (None, None)
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=ptr(controls, H * I), v_inout=None, u0=None,
                            iters=None)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=sp, residual_in=rip,
                        residual_out=rop)
        flags = C.c_uint32(0)
        self._check(self._lib.tpc_mpc_polish_batch_general(self._h, C.byref(p), C.byref(io), C.byref(q),
                                                           C.byref(flags) if want_status else None, mem, stream))
        self.last_flags = flags.value
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
        unknown = set(want) - set(self.GRAD_NAMES)
        if unknown:
            raise ValueError(f"unknown gradient names {sorted(unknown)}")
        if _is_torch(A):
            import torch
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, rows):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                    raise ValueError(f"expected contiguous fp64 CUDA tensor [{rows},{n}]")
                return t.data_ptr()

            def new(rows):
                return torch.empty((rows, n), dtype=torch.float64, device=A.device)
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
        else:
            A = np.ascontiguousarray(A, dtype=np.float64)
            n = A.shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, rows):
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (rows, n):
                    raise ValueError(f"expected an array [{rows},{n}]")
                keep.append(a)
                return a.ctypes.data

            def new(rows):
                return np.empty((rows, n), dtype=np.float64)
            stream = None
            mem = capi.HOST
        rows = {"A": 4, "B": 2 * I, "C": 2, "Q": 2, "R": I, "lower": I, "upper": I, "x0": 2, "targets": 2 * H,
                "kkt_residual": 1}
        out = {k: new(rows[k]) for k in want}

        def optr(k):
            if k not in out:
                return None
            return out[k].data_ptr() if mem == capi.DEVICE else out[k].ctypes.data
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=None, v_inout=None, u0=None, iters=None)
        g = capi.GeneralGrad(controls=ptr(controls, H * I), grad_controls=ptr(grad_controls, H * I),
                             dA=optr("A"), dB=optr("B"), dC=optr("C"), dQ=optr("Q"), dR=optr("R"),
                             dlower=optr("lower"), dupper=optr("upper"), dx0=optr("x0"), dtargets=optr("targets"),
                             kkt_residual=optr("kkt_residual"))
        flags = C.c_uint32(0)
        self._check(self._lib.tpc_mpc_solve_batch_general_backward(self._h, C.byref(p), C.byref(io), C.byref(g),
                                                                   C.byref(flags) if want_flags else None, mem, stream))
        self.last_flags = flags.value
        if "kkt_residual" in out:
            out["kkt_residual"] = out["kkt_residual"].reshape(n)
        return out

    def _plant(self, plant, disturbance, ptr, I, steps):
        """capi.Plant of plant=(Ap, Bp, Cp) | None and disturbance [steps*2, n] | None, through the call's ptr()."""
        if plant is not None and len(plant) != 3:
            raise ValueError("plant must be (Ap, Bp, Cp)")
        Ap, Bp, Cp = plant if plant is not None else (None, None, None)
        d = ptr(disturbance, 2 * steps)
        ld_d = 0 if disturbance is None else int(disturbance.shape[-1])
        return capi.Plant(A=ptr(Ap, 4), B=ptr(Bp, 2 * I), C=ptr(Cp, 2), disturbance=d, ld_d=ld_d)

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
        if _is_torch(A):
            import torch
            tdt = torch.float64 if p.dtype == capi.F64 else torch.float32
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, rows):
                if t is None:
                    return None
                if not (t.is_cuda and t.dtype == tdt and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                    raise ValueError(f"expected contiguous CUDA tensor [{rows},{n}] of the solver dtype")
                return t.data_ptr()
            c_out = torch.empty((steps * I, n), dtype=tdt, device=A.device)
            s_out = torch.empty((steps * 2, n), dtype=tdt, device=A.device) if want_states else None
            i_out = torch.empty((steps, n), dtype=torch.int32, device=A.device) if want_iters else None
            q_out = torch.empty((steps * H * I, n), dtype=tdt, device=A.device) if record else None
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
            optr = lambda t: None if t is None else t.data_ptr()
        else:
            dt = _NP[p.dtype]
            A = np.ascontiguousarray(A, dtype=dt)
            n = A.shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, rows):
                if a is None:
                    return None
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.shape == (rows, n)):
                    raise ValueError(f"expected C-contiguous ndarray [{rows},{n}] of the solver dtype")
                keep.append(a)
                return a.ctypes.data
            B, Cc, Q, R, lower, upper, x0, targets = (np.ascontiguousarray(a, dtype=dt) for a in
                                                      (B, Cc, Q, R, lower, upper, x0, targets))
            if new_last_targets is not None:
                new_last_targets = np.ascontiguousarray(new_last_targets, dtype=dt)
            c_out = np.empty((steps * I, n), dtype=dt)
            s_out = np.empty((steps * 2, n), dtype=dt) if want_states else None
            i_out = np.empty((steps, n), dtype=np.int32) if want_iters else None
            q_out = np.empty((steps * H * I, n), dtype=dt) if record else None
            stream = None
            mem = capi.HOST
            optr = lambda a: None if a is None else a.ctypes.data
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=ptr(controls, H * I),
                            v_inout=ptr(v_state, H * I), u0=None, iters=None)
        flags = C.c_uint32(0)
        if plant is not None or disturbance is not None:
            pl = self._plant(plant, disturbance, ptr, I, steps)
            self._check(self._lib.tpc_mpc_rollout_plant(self._h, C.byref(p), C.byref(io), C.byref(pl), capi.LOOP_RECORD,
                                                        int(steps), ptr(new_last_targets, 2 * steps), None, 0,
                                                        optr(c_out), optr(s_out), optr(i_out), optr(q_out), None,
                                                        C.byref(flags), mem, stream))
        elif record:
            self._check(self._lib.tpc_mpc_rollout_record(self._h, C.byref(p), C.byref(io), int(steps),
                                                         ptr(new_last_targets, 2 * steps), optr(c_out), optr(s_out),
                                                         optr(i_out), optr(q_out), C.byref(flags), mem, stream))
        else:
            self._check(self._lib.tpc_mpc_rollout(self._h, C.byref(p), C.byref(io), int(steps),
                                                  ptr(new_last_targets, 2 * steps), optr(c_out), optr(s_out),
                                                  optr(i_out), C.byref(flags), mem, stream))
        self.last_flags = flags.value
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
        p = self._params(**over)
        H = p.horizon
        if _is_torch(A):
            import torch
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, rows):
                if t is None:
                    return None
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                    raise ValueError(f"expected contiguous fp64 CUDA tensor [{rows},{n}]")
                return t.data_ptr()

            def new(rows, dtype=np.float64):
                return torch.empty((rows, n), dtype=torch.float64 if dtype is np.float64 else torch.int32,
                                   device=A.device)
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
            optr = lambda t: None if t is None else t.data_ptr()
        else:
            A = np.ascontiguousarray(A, dtype=np.float64)
            n = A.shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, rows):
                if a is None:
                    return None
                if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and
                        a.shape == (rows, n)):
                    raise ValueError(f"expected C-contiguous fp64 ndarray [{rows},{n}]")
                keep.append(a)
                return a.ctypes.data
            B, Cc, Q, R, lower, upper, x0, targets = (np.ascontiguousarray(a, dtype=np.float64) for a in
                                                      (B, Cc, Q, R, lower, upper, x0, targets))
            if new_last_targets is not None:
                new_last_targets = np.ascontiguousarray(new_last_targets, dtype=np.float64)

            def new(rows, dtype=np.float64):
                return np.empty((rows, n), dtype=dtype)
            stream = None
            mem = capi.HOST
            optr = lambda a: None if a is None else a.ctypes.data
        c_out, s_out, q_out = new(steps * I), new(steps * 2), new(steps * H * I)
        i_out = new(steps, np.int32) if want_iters else None
        status = new(steps, np.int32) if want_status else None
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=ptr(controls, H * I),
                            v_inout=ptr(v_state, H * I), u0=None, iters=None)
        rin, rout = residuals if residuals is not None else (None, None)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=optr(status),
                        residual_in=ptr(rin, steps), residual_out=ptr(rout, steps))
        flags = C.c_uint32(0)
        if plant is not None or disturbance is not None:   # the same loop against a separate plant
            pl = self._plant(plant, disturbance, ptr, I, steps)
            self._check(self._lib.tpc_mpc_rollout_plant(self._h, C.byref(p), C.byref(io), C.byref(pl),
                                                        capi.LOOP_POLISHED, int(steps),
                                                        ptr(new_last_targets, 2 * steps), C.byref(q), 0, optr(c_out),
                                                        optr(s_out), optr(i_out), optr(q_out), None,
                                                        C.byref(flags) if want_status else None, mem, stream))
            self.last_flags = flags.value
            return c_out, s_out, q_out, status, i_out
        self._check(self._lib.tpc_mpc_rollout_polished(self._h, C.byref(p), C.byref(io), int(steps),
                                                       ptr(new_last_targets, 2 * steps), C.byref(q), optr(c_out),
                                                       optr(s_out), optr(i_out), optr(q_out),
                                                       C.byref(flags) if want_status else None, mem, stream))
        self.last_flags = flags.value
        return c_out, s_out, q_out, status, i_out

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
        p = self._params(**over)
        H = p.horizon
        if _is_torch(A):
            import torch
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, rows):
                if t is None:
                    return None
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                    raise ValueError(f"expected contiguous fp64 CUDA tensor [{rows},{n}]")
                return t.data_ptr()

            def new(rows, dtype=np.float64):
                return torch.empty((rows, n), dtype=torch.float64 if dtype is np.float64 else torch.int32,
                                   device=A.device)
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
            optr = lambda t: None if t is None else t.data_ptr()
        else:
            A = np.ascontiguousarray(A, dtype=np.float64)
            n = A.shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, rows):
                if a is None:
                    return None
                if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and
                        a.shape == (rows, n)):
                    raise ValueError(f"expected C-contiguous fp64 ndarray [{rows},{n}]")
                keep.append(a)
                return a.ctypes.data
            B, Cc, Q, R, lower, upper, x0, targets = (np.ascontiguousarray(a, dtype=np.float64) for a in
                                                      (B, Cc, Q, R, lower, upper, x0, targets))
            if new_last_targets is not None:
                new_last_targets = np.ascontiguousarray(new_last_targets, dtype=np.float64)

            def new(rows, dtype=np.float64):
                return np.empty((rows, n), dtype=dtype)
            stream = None
            mem = capi.HOST
            optr = lambda a: None if a is None else a.ctypes.data
        c_out, s_out, q_out = new(steps * I), new(steps * 2), new(steps * H * I)
        i_out = new(steps, np.int32) if want_iters else None
        status = new(steps, np.int32) if want_status else None
        first = new(1, np.int32)
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=ptr(controls, H * I),
                            v_inout=ptr(v_state, H * I), u0=None, iters=None)
        rin, rout = residuals if residuals is not None else (None, None)
        q = capi.Polish(tol=float(tol), max_rounds=int(max_rounds), reserved=0, status=optr(status),
                        residual_in=ptr(rin, steps), residual_out=ptr(rout, steps))
        flags = C.c_uint32(0)
        if plant is not None or disturbance is not None:   # the same loop against a separate plant
            pl = self._plant(plant, disturbance, ptr, I, steps)
            self._check(self._lib.tpc_mpc_rollout_plant(self._h, C.byref(p), C.byref(io), C.byref(pl), capi.LOOP_NEWTON,
                                                        int(steps), ptr(new_last_targets, 2 * steps), C.byref(q),
                                                        capi.NEWTON_FALLBACKS[fallback], optr(c_out), optr(s_out),
                                                        optr(i_out), optr(q_out), optr(first),
                                                        C.byref(flags) if want_status else None, mem, stream))
            self.last_flags = flags.value
            return c_out, s_out, q_out, status, i_out, first[0]
        self._check(self._lib.tpc_mpc_rollout_newton(self._h, C.byref(p), C.byref(io), int(steps),
                                                     ptr(new_last_targets, 2 * steps), C.byref(q),
                                                     capi.NEWTON_FALLBACKS[fallback], optr(c_out), optr(s_out),
                                                     optr(i_out), optr(q_out), optr(first),
                                                     C.byref(flags) if want_status else None, mem, stream))
        self.last_flags = flags.value
        return c_out, s_out, q_out, status, i_out, first[0]

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
        unknown = set(want) - set(self.ROLLOUT_GRAD_NAMES) - set(self.PLANT_GRAD_NAMES)
        if unknown:
            raise ValueError(f"unknown gradient names {sorted(unknown)}")
        if _is_torch(A):
            import torch
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, rows):
                if t is None:
                    return None
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, n)):
                    raise ValueError(f"expected contiguous fp64 CUDA tensor [{rows},{n}]")
                return t.data_ptr()

            def new(rows):
                return torch.empty((rows, n), dtype=torch.float64, device=A.device)
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
        else:
            A = np.ascontiguousarray(A, dtype=np.float64)
            n = A.shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, rows):
                if a is None:
                    return None
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (rows, n):
                    raise ValueError(f"expected an array [{rows},{n}]")
                keep.append(a)
                return a.ctypes.data

            def new(rows):
                return np.empty((rows, n), dtype=np.float64)
            stream = None
            mem = capi.HOST
        rows = {"A": 4, "B": 2 * I, "C": 2, "Q": 2, "R": I, "lower": I, "upper": I, "x0": 2, "targets": 2 * H,
                "new_last_targets": 2 * steps, "kkt_residual": 1, "Ap": 4, "Bp": 2 * I, "Cp": 2,
                "disturbance": 2 * steps}
        out = {k: new(rows[k]) for k in want}

        def optr(k):
            if k not in out:
                return None
            return out[k].data_ptr() if mem == capi.DEVICE else out[k].ctypes.data
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=None, v_inout=None, u0=None, iters=None)
        g = capi.RolloutGrad(sequences=ptr(sequences, steps * H * I), states=ptr(states, 2 * steps),
                             grad_controls=ptr(grad_controls, steps * I), grad_states=ptr(grad_states, 2 * steps),
                             dA=optr("A"), dB=optr("B"), dC=optr("C"), dQ=optr("Q"), dR=optr("R"),
                             dlower=optr("lower"), dupper=optr("upper"), dx0=optr("x0"), dtargets=optr("targets"),
                             dnew_last_targets=optr("new_last_targets"), kkt_residual=optr("kkt_residual"))
        flags = C.c_uint32(0)
        if plant_call:
            pl = self._plant(plant, None, ptr, I, steps)   # (the disturbance itself is not read: the states are recorded)
            pg = capi.PlantGrad(dA=optr("Ap"), dB=optr("Bp"), dC=optr("Cp"), ddisturbance=optr("disturbance"))
            self._check(self._lib.tpc_mpc_rollout_plant_backward(self._h, C.byref(p), C.byref(io), C.byref(pl),
                                                                 int(steps), ptr(new_last_targets, 2 * steps),
                                                                 C.byref(g), C.byref(pg),
                                                                 C.byref(flags) if want_flags else None, mem, stream))
            self.last_flags = flags.value
            if "kkt_residual" in out:
                out["kkt_residual"] = out["kkt_residual"].reshape(n)
            return out
        self._check(self._lib.tpc_mpc_rollout_backward(self._h, C.byref(p), C.byref(io), int(steps),
                                                       ptr(new_last_targets, 2 * steps), C.byref(g),
                                                       C.byref(flags) if want_flags else None, mem, stream))
        self.last_flags = flags.value
        if "kkt_residual" in out:
            out["kkt_residual"] = out["kkt_residual"].reshape(n)
        return out

    TANGENT_NAMES = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "new_last_targets")
    PLANT_TANGENT_NAMES = ("Ap", "Bp", "Cp", "disturbance")

    def _forward_setup(self, A, R, inputs, tangents, rows):
        """What the two forward-mode calls share: (n, I, K, ptr, new, stream, mem, Tangents factory).  `tangents` maps
        names of TANGENT_NAMES (and PLANT_TANGENT_NAMES -> the PlantTangents struct) to arrays [K, c, n] (2-D [c, n]: K = 1);
        rows(I) gives c per name."""
        unknown = set(tangents) - set(self.TANGENT_NAMES) - set(self.PLANT_TANGENT_NAMES)
        if unknown:
            raise ValueError(f"unknown tangent names {sorted(unknown)}")
        tangents = {k: v for k, v in tangents.items() if v is not None}
        if not tangents:
            raise ValueError("tangents is empty: give at least one direction array")
        K = None
        for name, v in tangents.items():
            k = 1 if v.ndim == 2 else v.shape[0] if v.ndim == 3 else None
            if k is None or (K is not None and k != K):
                raise ValueError(f"tangent {name!r}: expected [K, c, n] (or [c, n] for K = 1) with one K for all")
            K = k
        if _is_torch(A):
            import torch
            n = A.shape[-1]
            I = inputs or R.shape[0]

            def ptr(t, r):
                if t is None:
                    return None
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == r * n
                        and t.shape[-1] == n):
                    raise ValueError(f"expected contiguous fp64 CUDA tensor [{r},{n}]")
                return t.data_ptr()

            def new(*shape):
                return torch.empty(shape + (n,), dtype=torch.float64, device=A.device)
            stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
            mem = capi.DEVICE
            optr = lambda t: None if t is None else t.data_ptr()
        else:
            n = np.asarray(A).shape[-1]
            I = inputs or np.asarray(R).shape[0]
            keep = []

            def ptr(a, r):
                if a is None:
                    return None
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.size != r * n or a.shape[-1] != n:
                    raise ValueError(f"expected an array [{r},{n}]")
                keep.append(a)
                return a.ctypes.data

            def new(*shape):
                return np.empty(shape + (n,), dtype=np.float64)
            stream = None
            mem = capi.HOST
            optr = lambda a: None if a is None else a.ctypes.data
        c = rows(I)
        fields = {("t" + name): ptr(tangents.get(name), K * c[name]) for name in self.TANGENT_NAMES}
        tan = capi.Tangents(directions=K, reserved=0, **fields)
        ptan = capi.PlantTangents(
            tA=ptr(tangents.get("Ap"), K * 4), tB=ptr(tangents.get("Bp"), K * 2 * I), tC=ptr(tangents.get("Cp"), K * 2),
            tdisturbance=ptr(tangents.get("disturbance"), K * c.get("disturbance", 0)))
        return n, I, K, ptr, new, optr, stream, mem, tan, ptan

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
        n, I, K, ptr, new, optr, stream, mem, tan, ptan = self._forward_setup(
            A, R, inputs, tangents, lambda I: {"A": 4, "B": 2 * I, "C": 2, "Q": 2, "R": I, "lower": I, "upper": I,
                                               "x0": 2, "targets": 2 * H, "new_last_targets": 0})
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=None, v_inout=None, u0=None, iters=None)
        tu = new(K, H * I)
        flags = C.c_uint32(0)
        self._check(self._lib.tpc_mpc_solve_batch_general_forward(self._h, C.byref(p), C.byref(io),
                                                                  ptr(controls, H * I), C.byref(tan), optr(tu),
                                                                  C.byref(flags) if want_flags else None, mem, stream))
        self.last_flags = flags.value
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
        n, I, K, ptr, new, optr, stream, mem, tan, ptan = self._forward_setup(
            A, R, inputs, tangents, lambda I: {"A": 4, "B": 2 * I, "C": 2, "Q": 2, "R": I, "lower": I, "upper": I,
                                               "x0": 2, "targets": 2 * H, "new_last_targets": 2 * steps,
                                               "disturbance": 2 * steps})
        io = capi.GeneralIO(inputs=I, n=n, ld=n, A=ptr(A, 4), B=ptr(B, 2 * I), C=ptr(Cc, 2), Q=ptr(Q, 2),
                            R=ptr(R, I), lower=ptr(lower, I), upper=ptr(upper, I), x0=ptr(x0, 2),
                            targets=ptr(targets, 2 * H), controls_inout=None, v_inout=None, u0=None, iters=None)
        tu = new(K, steps * I)
        tx = new(K, steps * 2) if want_states else None
        flags = C.c_uint32(0)
        if plant_call:
            pl = self._plant(plant, None, ptr, I, steps)   # (the disturbance itself is not read: the states are recorded)
            self._check(self._lib.tpc_mpc_rollout_plant_forward(self._h, C.byref(p), C.byref(io), C.byref(pl), int(steps),
                                                                ptr(new_last_targets, 2 * steps),
                                                                ptr(sequences, steps * H * I), ptr(states, 2 * steps),
                                                                C.byref(tan), C.byref(ptan), optr(tu),
                                                                optr(tx), C.byref(flags) if want_flags else None, mem,
                                                                stream))
            self.last_flags = flags.value
            return tu, tx
        self._check(self._lib.tpc_mpc_rollout_forward(self._h, C.byref(p), C.byref(io), int(steps),
                                                      ptr(new_last_targets, 2 * steps),
                                                      ptr(sequences, steps * H * I), ptr(states, 2 * steps),
                                                      C.byref(tan), optr(tu), optr(tx),
                                                      C.byref(flags) if want_flags else None, mem, stream))
        self.last_flags = flags.value
        return tu, tx

    def follow_batch(self, pos_x, pos_y, dir_x, dir_y, velocity, count, car_velocity, look_ahead,
                     lookup=None, want_iters: bool = False, **over):
        """Batched tobiMPC branch of cycle() on raw trajectories (device tensors).

        pos_x .. velocity: float32 CUDA tensors [max_points, n] (point-major, SoA); count int32 [n];
        car_velocity, look_ahead float32 [n]; lookup: optional (x, y) float32 CUDA tensors of the
        velocity lookup table.  Returns (steering_front f64, steering_rear f64, target_speed f32,
        target_distance f32[, iters])."""
        import torch
        p = self._params(**over)
        P, n = pos_x.shape
        dev = pos_x.device
        for tns in (pos_x, pos_y, dir_x, dir_y, velocity):
            if not (tns.is_cuda and tns.dtype == torch.float32 and tns.is_contiguous() and tuple(tns.shape) == (P, n)):
                raise ValueError("trajectory arrays must be contiguous float32 CUDA tensors [max_points, n]")
        for tns, dt in ((count, torch.int32), (car_velocity, torch.float32), (look_ahead, torch.float32)):
            if not (tns.is_cuda and tns.dtype == dt and tns.is_contiguous() and tns.numel() == n):
                raise ValueError("per-instance arrays must be contiguous CUDA tensors of length n")
        tr = capi.Trajectories(n=n, ld=n, max_points=P, pos_x=pos_x.data_ptr(), pos_y=pos_y.data_ptr(),
                               dir_x=dir_x.data_ptr(), dir_y=dir_y.data_ptr(), velocity=velocity.data_ptr(),
                               count=count.data_ptr(), car_velocity=car_velocity.data_ptr(),
                               look_ahead=look_ahead.data_ptr())
        front = torch.empty(n, dtype=torch.float64, device=dev)
        rear = torch.empty(n, dtype=torch.float64, device=dev)
        tspeed = torch.empty(n, dtype=torch.float32, device=dev)
        tdist = torch.empty(n, dtype=torch.float32, device=dev)
        iters = torch.empty(n, dtype=torch.int32, device=dev) if want_iters else None
        lx, ly, ln = (None, None, 0) if lookup is None else (lookup[0].data_ptr(), lookup[1].data_ptr(), lookup[0].numel())
        flags = C.c_uint32(0)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self._check(self._lib.tpc_mpc_follow_batch(self._h, C.byref(p), C.byref(tr), lx, ly, ln,
                                                   front.data_ptr(), rear.data_ptr(), tspeed.data_ptr(),
                                                   tdist.data_ptr(), iters.data_ptr() if want_iters else None,
                                                   C.byref(flags), stream))
        self.last_flags = flags.value
        return (front, rear, tspeed, tdist, iters) if want_iters else (front, rear, tspeed, tdist)

    def follow_batch_horizon(self, pos_x, pos_y, dir_x, dir_y, velocity, count, car_velocity, look_ahead,
                             step_spacing=None, lookup=None, want_iters: bool = False,
                             want_targets: bool = False, **over):
        """follow_batch with one trajectory point per horizon step (tpc_mpc_follow_batch_horizon):
        step t's target is the polyline point at arc length look_ahead + t * spacing.  step_spacing:
        optional float32 CUDA tensor [n] (None: |v| * step_size).  Returns (front, rear, target_speed,
        target_distance[, targets f64 [2H, n]][, iters])."""
        import torch
        p = self._params(**over)
        P, n = pos_x.shape
        dev = pos_x.device
        for tns in (pos_x, pos_y, dir_x, dir_y, velocity):
            if not (tns.is_cuda and tns.dtype == torch.float32 and tns.is_contiguous() and tuple(tns.shape) == (P, n)):
                raise ValueError("trajectory arrays must be contiguous float32 CUDA tensors [max_points, n]")
        per = [(count, torch.int32), (car_velocity, torch.float32), (look_ahead, torch.float32)]
        if step_spacing is not None:
            per.append((step_spacing, torch.float32))
        for tns, dt in per:
            if not (tns.is_cuda and tns.dtype == dt and tns.is_contiguous() and tns.numel() == n):
                raise ValueError("per-instance arrays must be contiguous CUDA tensors of length n")
        tr = capi.Trajectories(n=n, ld=n, max_points=P, pos_x=pos_x.data_ptr(), pos_y=pos_y.data_ptr(),
                               dir_x=dir_x.data_ptr(), dir_y=dir_y.data_ptr(), velocity=velocity.data_ptr(),
                               count=count.data_ptr(), car_velocity=car_velocity.data_ptr(),
                               look_ahead=look_ahead.data_ptr())
        front = torch.empty(n, dtype=torch.float64, device=dev)
        rear = torch.empty(n, dtype=torch.float64, device=dev)
        tspeed = torch.empty(n, dtype=torch.float32, device=dev)
        tdist = torch.empty(n, dtype=torch.float32, device=dev)
        targets = torch.empty((2 * p.horizon, n), dtype=torch.float64, device=dev) if want_targets else None
        iters = torch.empty(n, dtype=torch.int32, device=dev) if want_iters else None
        lx, ly, ln = (None, None, 0) if lookup is None else (lookup[0].data_ptr(), lookup[1].data_ptr(), lookup[0].numel())
        flags = C.c_uint32(0)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self._check(self._lib.tpc_mpc_follow_batch_horizon(
            self._h, C.byref(p), C.byref(tr), step_spacing.data_ptr() if step_spacing is not None else None,
            lx, ly, ln, front.data_ptr(), rear.data_ptr(), tspeed.data_ptr(), tdist.data_ptr(),
            targets.data_ptr() if want_targets else None, iters.data_ptr() if want_iters else None,
            C.byref(flags), stream))
        self.last_flags = flags.value
        out = [front, rear, tspeed, tdist]
        if want_targets:
            out.append(targets)
        if want_iters:
            out.append(iters)
        return tuple(out)
