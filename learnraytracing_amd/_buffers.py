"""What the post-process front ends of renderer.py need of a caller's buffers, once for NumPy arrays
(HostBuffers -> the library's lrt_*_host entries) and once for cuda tensors (TensorBuffers ->
lrt_*_device, on a stream). Both expose

    check(buf, what, count, dtypes=("float32",), exact=False)   LrtError(LRT_E_INVALID) unless it fits
    check_plane(buf, what, plane, exact=False)                   the same for a plane of planes(w, h)
    ptr(buf)                                                     its address as c_void_p; None for None
    address(buf)                                                 its address as an int, for a struct member
    zeros(shape, dtype), copy(buf)                               a new buffer (tensors: on the stream)
    entry(unit)                                                  lrt_<unit>_host or lrt_<unit>_device
    tail                                                         the arguments after the buffers: the stream
    uword                                                        the dtype of unsigned 32-bit words

so that a unit's marshalling is written once, taking either. Dtypes travel by name ("float32",
"int32", ...). torch is imported by TensorBuffers alone: the package needs none."""
from __future__ import annotations

import ctypes
import numpy as np

from . import _lib as L


# A plane of a frame is the plain tuple (element count, the dtype names it may have -- a new one gets
# the first --, shape): plain because the front ends build the table below on every call.
def planes(width: int, height: int) -> dict:
    """The plane kinds of a width x height frame: RGBA quads, int32 words (ids, keys, classes) and
    float scalars (depth)."""
    w, h = int(width), int(height)
    return {"quad": (w * h * 4, _F32, (h, w, 4)), "word": (w * h, _I32, (h, w)), "scalar": (w * h, _F32, (h, w))}


_F32, _I32 = ("float32",), ("int32",)


def _invalid(what, kind, dtypes, count, exact):
    return L.LrtError(L.LRT_E_INVALID, f"{what} must be a {kind[0]} {dtypes[0]} {kind[1]} of "
                                       f"{'' if exact else '>= '}{count} elements")


class _Buffers:
    # The checks run per frame and per buffer, and a Python call per check shows in the per-call host
    # time (profiles/r15_front_ends/README.md): so check_plane is one call deep, and the dtype objects
    # behind the names are looked up once per back end (`_native`).
    def check(self, buf, what, count, dtypes=("float32",), exact=False) -> None:
        self.check_plane(buf, what, (count, tuple(dtypes), None), exact)

    def new(self, plane):
        """A zeroed plane."""
        return self.zeros(plane[2], plane[1][0])


class HostBuffers(_Buffers):
    """NumPy arrays in host memory."""
    tail = ()
    uword = "uint32"
    _native = {}

    def check_plane(self, buf, what, plane, exact=False) -> None:
        count, dtypes = plane[0], plane[1]
        try:
            native = self._native[dtypes]
        except KeyError:
            native = self._native[dtypes] = tuple(np.dtype(name) for name in dtypes)
        if not (isinstance(buf, np.ndarray) and buf.dtype in native and buf.flags.c_contiguous
                and (buf.size == count if exact else buf.size >= count)):
            raise _invalid(what, ("C-contiguous", "array"), dtypes, count, exact)

    def ptr(self, buf):
        return ctypes.c_void_p(buf.ctypes.data) if buf is not None else None

    def address(self, buf) -> int:
        return buf.ctypes.data

    def zeros(self, shape, dtype="float32"):
        return np.zeros(shape, dtype)

    def copy(self, buf):
        return buf.copy()

    def entry(self, unit: str):
        return getattr(L.lib(), f"lrt_{unit}_host")


class TensorBuffers(_Buffers):
    """Contiguous cuda tensors on one device; the work, and every fill of a new buffer, goes to
    `stream` (a torch.cuda.Stream; None: the device's current one)."""
    uword = "int32"        # torch's uint32 is recent and partial: the words travel as int32
    _native = {}

    def __init__(self, device, stream=None):
        import torch

        self.torch = torch
        self.device = device if isinstance(device, torch.device) else torch.device(device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.tail = (ctypes.c_void_p(self.stream.cuda_stream),)

    def check_plane(self, buf, what, plane, exact=False) -> None:
        count, dtypes = plane[0], plane[1]
        try:
            native = self._native[dtypes]
        except KeyError:
            native = self._native[dtypes] = tuple(getattr(self.torch, name, None) for name in dtypes)
        if not (isinstance(buf, self.torch.Tensor) and buf.is_cuda and buf.device == self.device
                and buf.dtype in native and buf.is_contiguous()
                and (buf.numel() == count if exact else buf.numel() >= count)):
            raise _invalid(what, ("contiguous cuda", "tensor"), dtypes, count, exact)

    def ptr(self, buf):
        return ctypes.c_void_p(buf.data_ptr()) if buf is not None else None

    def address(self, buf) -> int:
        return buf.data_ptr()

    def zeros(self, shape, dtype="float32"):
        with self.torch.cuda.stream(self.stream):
            return self.torch.zeros(shape, dtype=getattr(self.torch, dtype), device=self.device)

    def copy(self, buf):
        with self.torch.cuda.stream(self.stream):
            return buf.clone()

    def entry(self, unit: str):
        return getattr(L.lib(), f"lrt_{unit}_device")


def tensor_buffers(key, what: str, count: int, stream=None, dtype: str = "float32") -> TensorBuffers:
    """The TensorBuffers of the tensor a unit keys on (its device is every other buffer's), `what` of
    >= count elements; anything but a cuda tensor -- a NumPy array, say -- is LRT_E_INVALID."""
    import torch

    if not (isinstance(key, torch.Tensor) and key.is_cuda):
        raise _invalid(what, ("contiguous cuda", "tensor"), (dtype,), count, False)
    return TensorBuffers(key.device, stream)
