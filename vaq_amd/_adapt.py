"""What the adapter modules (single, fast, refiner, multi, fits, merge) share: pointers, the checks of byte rows,
identity tokens of uploaded members, the output pair and the stream of a device call, a ctypes structure as a dict,
and the lifetime of a C handle.  Nothing here computes."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _dptr(t):
    """The address a torch tensor starts at."""
    return C.c_void_p(t.data_ptr())


def _f32_rows(X, D: int, what: str) -> np.ndarray:
    """X as contiguous float32 rows of D columns; `what` is the refusal's text up to the shape ("rows {shape} are
    not n x D", "XTest {shape} is not nq x D": every site keeps its own)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2 or X.shape[1] != D:
        raise _lib.VaqHipError(-1, what.format(shape=X.shape, D=D))
    return X


def _u8_rows(X, D: int) -> np.ndarray:
    """Byte rows as the *_u8 calls take them: a contiguous uint8 n x D array; anything else is EINVAL, nothing is
    converted."""
    X = np.asarray(X)
    if X.dtype != np.uint8 or X.ndim != 2 or X.shape[1] != D or not X.flags.c_contiguous:
        raise _lib.VaqHipError(-1, f"byte rows must be a contiguous uint8 n x {D} array (nothing is converted)")
    return X


def _u8_rows_device(d_X, D: int):
    """The same for a torch CUDA tensor; a view that starts at any byte of its allocation is taken as it is."""
    import torch
    if not (d_X.is_cuda and d_X.dtype == torch.uint8 and d_X.dim() == 2 and d_X.shape[1] == D and d_X.is_contiguous()):
        raise _lib.VaqHipError(-1, f"byte rows must be a contiguous uint8 n x {D} CUDA tensor (nothing is converted)")
    return d_X


def _wref(obj):
    """Identity token of a member that was uploaded: a weak reference (an id() can be recycled
    by a new array once the old one is freed; a dead weak reference never compares alive)."""
    if obj is None:
        return None
    try:
        return weakref.ref(obj)
    except TypeError:  # plain lists / tuples: fall back to the object itself (small)
        return lambda o=obj: o


def _same(ref, obj) -> bool:
    if ref is None or obj is None:
        return ref is None and obj is None
    return ref() is obj


def _eig_f32(eigvec, D: int, name: str):
    """The real part of a D x D rotation as contiguous float32, or None."""
    if eigvec is None:
        return None
    eig = np.ascontiguousarray(np.real(eigvec), dtype=np.float32)
    if eig.shape != (D, D):
        raise _lib.VaqHipError(-1, f"{name} {eig.shape} is not {D}x{D}")
    return eig


def _out_pair(out, nq: int, k: int, device):
    """(labels int32 [nq, k], dists float32 [nq, k]) of a device call: the caller's `out`, or new tensors."""
    if out is not None:
        return out
    import torch
    return (torch.empty((nq, k), dtype=torch.int32, device=device),
            torch.empty((nq, k), dtype=torch.float32, device=device))


def _torch_stream(device):
    import torch
    return torch.cuda.current_stream(device)


def _stream(t):
    """The handle of torch's stream in force on tensor t's device, as the *_device calls take it."""
    return C.c_void_p(_torch_stream(t.device).cuda_stream)


def _struct_dict(st, cut=()) -> dict:
    """A ctypes structure as a dict in field order; array fields become lists, those named in `cut` only their
    first n_devices entries."""
    d = {}
    for f, _ in st._fields_:
        v = getattr(st, f)
        if isinstance(v, C.Array):
            v = list(v)[:st.n_devices] if f in cut else list(v)
        d[f] = v
    return d


class _Handle:
    """The lifetime of the C object behind self._h; the subclass names the symbol that destroys it."""
    _destroy = ""

    def close(self) -> None:
        if self._h:
            getattr(_lib.load(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
