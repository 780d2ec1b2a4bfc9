"""Where one MpcSolver call's arrays live: `Arrays`, the one place that tells numpy from CUDA tensors.

One rule for every entry: an array the library only reads is coerced on the numpy side (np.ascontiguousarray to the
wanted dtype, then shape-checked, kept alive until the call returns); an array the library writes into never is, since a
coerced copy would swallow the result; a tensor is never copied -- it must be a contiguous CUDA tensor of the dtype and
shape.  Anything else is a ValueError here, before a pointer reaches the library.  Needs no library and no torch.

How an array is matched against the call's n: "shape" is [rows, n] exactly ([n] without rows), "loose" (the forward-mode
arrays) leaves the leading dimensions free -- rows * n elements, last dimension n -- and "length" (the compact entries'
vectors) asks for n elements only; "elems" is an array that is not per instance (the shared parameters' tangent):
`rows` elements in all, whatever n is.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

NP_DTYPE = {capi.F64: np.float64, capi.F32: np.float32}
_TORCH_DTYPE = {}   # numpy dtype -> torch dtype, filled at the first tensor call
COUNT, LAST = None, -1   # Arrays(first, n): n instances = first's element count / first's last dimension


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _address(a):
    """a.ctypes.data, at a quarter of its cost where ctypes can take the buffer itself (a writable, non-empty array):
    the address is most of what binding a numpy array costs"""
    if a.flags.writeable and a.size:
        return C.addressof(C.c_char.from_buffer(a))
    return a.ctypes.data


def _raw_stream(torch, t):
    """torch.cuda.current_stream(t.device).cuda_stream; without building the Stream object where torch has the getter
    for it (about a microsecond of every small call)"""
    get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    return get(t.get_device()) if get is not None else torch.cuda.current_stream(t.device).cuda_stream


def _fits(shape, size, rows, n, match):
    """the one shape rule; read_rows spells its "shape" and "length" cases out inline, for speed"""
    if match == "shape":
        return shape == ((n,) if rows is None else (rows, n))
    if match == "length":
        return size == n
    if match == "elems":
        return size == rows
    return size == rows * n and len(shape) >= 1 and shape[-1] == n


class Arrays:
    """The memory kind of one call, taken from its first array: `mem` (capi.HOST / capi.DEVICE), `stream` (torch's
    current stream of that tensor's device, read now; None for numpy), `n` (the instances: given, COUNT or LAST) and
    `dtype`, the numpy dtype read / update / new default to (capi.F64 / capi.F32 are accepted).  `keep` holds the
    call's coerced arrays until it returns."""
    __slots__ = ("n", "dtype", "mem", "stream", "keep", "_torch", "_device", "_like")

    def __init__(self, first, n=COUNT, dtype=np.float64, like=False):
        """like: a DEVICE call's plain new() is torch.empty_like(first), as the compact and mixed entries always made
        their outputs (half the cost of torch.empty)"""
        self.dtype = NP_DTYPE.get(dtype, dtype)
        self.keep = []
        if type(first) is not np.ndarray and _is_torch(first):
            import torch
            if not _TORCH_DTYPE:
                _TORCH_DTYPE.update({np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32})
            if not first.is_cuda:
                raise ValueError("tensors must be CUDA tensors (host memory is passed as numpy arrays)")
            self._torch, self._device = torch, first.device
            self._like = first if like else None
            self.n = first.numel() if n is None else first.shape[-1] if n == LAST else int(n)
            self.mem = capi.DEVICE
            self.stream = C.c_void_p(_raw_stream(torch, first))
        else:
            self._torch = None
            a = first if type(first) is np.ndarray else np.asarray(first)   # (np.size / np.shape cost a microsecond)
            self.n = a.size if n is None else a.shape[-1] if n == LAST else int(n)
            self.mem = capi.HOST
            self.stream = None

    def _want(self, rows, dtype, match):
        shape = {"length": f"of {self.n} elements", "elems": f"of {rows} elements", "loose": f"[..., {self.n}] of {rows} x {self.n} elements"}.get(
            match, f"[{self.n}]" if rows is None else f"[{rows}, {self.n}]")
        return f"{np.dtype(dtype).name} {shape}"

    def read(self, a, rows=None, dtype=None, match="shape", convert=False):
        """Address of an array the library only reads, None for None.  convert: a DEVICE call takes anything
        torch.as_tensor does and moves it to the device and the dtype (the mixed entry's horizons)."""
        if a is None:
            return None
        if dtype is None:
            dtype = self.dtype
        if self._torch:
            if convert:
                a = self._torch.as_tensor(a, device=self._device).to(_TORCH_DTYPE[dtype]).contiguous()
                self.keep.append(a)
            return self._tensor(a, rows, dtype, match)
        a = np.ascontiguousarray(a, dtype=dtype)
        if not _fits(a.shape, a.size, rows, self.n, match):
            raise ValueError(f"expected an array {self._want(rows, dtype, match)}, got {list(a.shape)}")
        self.keep.append(a)
        return _address(a)

    def read_rows(self, arrays, rows=None, match="shape"):
        """[read(a, r, None, match) for a, r in zip(arrays, rows)] without a call per array (rows=None with "length"):
        the nine model arrays of the general form and the three vectors of the compact one are most of what a call
        binds, and this loop is most of a small call's cost."""
        rows = rows or (None,) * len(arrays)
        if match == "loose":
            return [self.read(a, r, None, match) for a, r in zip(arrays, rows)]
        n, dtype, length, keep, out = self.n, self.dtype, match == "length", self.keep, []
        if self._torch:
            tdt = _TORCH_DTYPE[dtype]
            for a, r in zip(arrays, rows):
                if a is None:
                    out.append(None)
                    continue
                if not (getattr(a, "is_cuda", False) and a.dtype == tdt and a.is_contiguous()
                        and (a.numel() == n if length else a.shape == (r, n))):
                    raise ValueError(f"expected a contiguous CUDA tensor {self._want(r, dtype, match)}")
                out.append(a.data_ptr())
            return out
        for a, r in zip(arrays, rows):
            if a is None:
                out.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.size != n if length else a.shape != (r, n):
                raise ValueError(f"expected an array {self._want(r, dtype, match)}, got {list(a.shape)}")
            keep.append(a)
            out.append(_address(a))
        return out

    def update(self, a, rows=None, dtype=None, match="shape"):
        """Address of an array the library writes into, None for None: never coerced."""
        if a is None:
            return None
        if dtype is None:
            dtype = self.dtype
        if self._torch:
            return self._tensor(a, rows, dtype, match)
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous
                and _fits(a.shape, a.size, rows, self.n, match)):
            raise ValueError(f"expected a C-contiguous ndarray {self._want(rows, dtype, match)} (it is written in place)")
        return _address(a)

    def _tensor(self, t, rows, dtype, match):
        if not (getattr(t, "is_cuda", False) and t.dtype == _TORCH_DTYPE[dtype] and t.is_contiguous()
                and _fits(t.shape, t.numel(), rows, self.n, match)):
            raise ValueError(f"expected a contiguous CUDA tensor {self._want(rows, dtype, match)}")
        return t.data_ptr()

    def new(self, *lead, dtype=None, per_instance=True):
        """A fresh output of the inputs' kind, shape lead + (n,) (per_instance=False: lead alone)."""
        if self._torch:
            if not lead and dtype is None and per_instance and self._like is not None:
                return self._torch.empty_like(self._like)
            return self._torch.empty(lead + (self.n,) if per_instance else lead, dtype=_TORCH_DTYPE[dtype or self.dtype],
                                     device=self._device)
        return np.empty(lead + (self.n,) if per_instance else lead, dtype=dtype or self.dtype)

    def addr(self, x):
        """Address of what new() made, None for None."""
        if x is None:
            return None
        return x.data_ptr() if self._torch else _address(x)
