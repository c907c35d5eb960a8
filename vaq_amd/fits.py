"""The fits that need no index: the subspace codebooks (vaqhip_fit_codebooks*, vaqhip_multi_fit_codebooks*) and
binaryEncodingLUT's quantile codebooks over several devices (vaqhip_multi_lut_fit_quantiles*), with their timing
calls.  The byte-row form of a fit is the float form's body with the other symbol."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._adapt import _eig_f32, _ptr, _struct_dict, _u8_rows


def _fit_rows(X, u8: bool) -> np.ndarray:
    """The n x D rows of a fit: float32 (anything is converted), or bytes as _u8_rows takes them."""
    if u8:
        X = np.asarray(X)
        return _u8_rows(X, X.shape[1] if X.ndim == 2 else 0)
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise _lib.VaqHipError(-1, f"X {X.shape} is not n x D")
    return X


def _device_list(devices):
    devs = [int(d) for d in devices]
    return len(devs), (C.c_int * max(len(devs), 1))(*devs)


def _fit_codebooks_call(D: int, M: int, bits, eigvec, max_iter: int, call, multi: bool = False):
    """The arrays around a vaqhip_*fit_codebooks call: ([M centre matrices k_s x L], iterations[M], nan_rows[M]).
    multi: a sharded call, whose error text is vaqhip_multi_last_error's."""
    bits = [int(b) for b in bits]
    M = int(M)
    if M < 1 or len(bits) != M or D % M != 0:
        raise _lib.VaqHipError(-1, f"{len(bits)} bits for M = {M} subspaces of D = {D}")
    eig = _eig_f32(eigvec, D, "eigvec")
    L_ = D // M
    ks = [1 << b if 0 < b < 31 else 0 for b in bits]  # (bits out of range: the call refuses them, nothing is written)
    cent = np.empty(max(sum(ks) * L_, 1), np.float32)
    iters = np.zeros(M, np.int32)
    nan_rows = np.zeros(M, np.int32)
    (_lib.check_multi if multi else _lib.check)(call(_lib.load(), (C.c_int * M)(*bits), _ptr(eig) if eig is not None else None,
                                                     int(max_iter), _ptr(cent), _ptr(iters), _ptr(nan_rows)))
    offs = np.concatenate([[0], np.cumsum(ks)]) * L_
    return [cent[offs[s]:offs[s + 1]].reshape(ks[s], L_).copy() for s in range(M)], iters, nan_rows


def _fit_codebooks(X, M, bits, eigvec, max_iter, device, devices, u8: bool):
    X = _fit_rows(X, u8)
    tail = "_u8" if u8 else ""
    if devices is not None:
        n_dev, arr = _device_list(devices)
        return _fit_codebooks_call(X.shape[1], M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: getattr(
            L, "vaqhip_multi_fit_codebooks" + tail)(n_dev, arr, _ptr(X), X.shape[0], X.shape[1], int(M), b, e, it, c, i, nn),
            multi=True)
    return _fit_codebooks_call(X.shape[1], M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: getattr(
        L, "vaqhip_fit_codebooks" + tail)(int(device), _ptr(X), X.shape[0], X.shape[1], int(M), b, e, it, c, i, nn))


def fit_codebooks(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25, device: int = 0,
                  devices: Optional[Sequence[int]] = None):
    """vaqhip_fit_codebooks: the subspace codebooks mCentroidsPerSubs by KMeans::staticFitSampling (the call of
    VAQ.cpp:644-649; not the arma::kmeans call VAQ::train runs today), every subspace fitted on the device, bit for
    bit the reference's.  X: n x D rows (unprojected when eigvec is given, else in PCA space); bits[M].  Returns
    ([M arrays (1 << bits[s]) x L], iterations[M], nan_rows[M]).  devices=[...]: the same result from the sharded fit
    (vaqhip_multi_fit_codebooks): the rows are cut over the devices, subspace s is fitted on devices[s % G] and no
    device holds all rows; a device named several times gives logical shards on that GPU."""
    return _fit_codebooks(X, M, bits, eigvec, max_iter, device, devices, False)


def fit_codebooks_u8(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25, device: int = 0,
                     devices: Optional[Sequence[int]] = None):
    """fit_codebooks from byte rows (vaqhip_fit_codebooks_u8, or vaqhip_multi_fit_codebooks_u8 with devices): the result
    is fit_codebooks's on X.astype(float32), bit for bit.  Anything but a contiguous uint8 n x D array is EINVAL."""
    return _fit_codebooks(X, M, bits, eigvec, max_iter, device, devices, True)


def fit_codebooks_timing(on: bool) -> None:
    """Phase times for the calling thread's fits (vaqhip_fit_codebooks_set_timing): one synchronisation per phase."""
    _lib.check(_lib.load().vaqhip_fit_codebooks_set_timing(1 if on else 0))


def last_fit_codebooks_timing() -> dict:
    """Figures of the calling thread's last codebook fit (vaqhip_last_fit_codebooks_timing)."""
    t = _lib.FitCodebooksTiming()
    _lib.check(_lib.load().vaqhip_last_fit_codebooks_timing(C.byref(t)))
    return _struct_dict(t)


def last_multi_fit_codebooks_timing() -> dict:
    """Figures of the calling thread's last sharded codebook fit (vaqhip_multi_last_fit_codebooks_timing); the owners'
    assign / accumulate / update times only under fit_codebooks_timing(True)."""
    t = _lib.MultiFitCodebooksTiming()
    _lib.check_multi(_lib.load().vaqhip_multi_last_fit_codebooks_timing(C.byref(t)))
    return _struct_dict(t, cut=("owner_subspaces",))


def _fit_quantiles_call(D: int, bits, eigvec, call):
    bits = [int(b) for b in bits]
    if len(bits) != D:
        raise _lib.VaqHipError(-1, f"{len(bits)} bits for D = {D}")
    eig = _eig_f32(eigvec, D, "eigvec")
    cent = np.empty((D, 256), np.float32)
    q = np.empty((D, 257), np.float32)
    _lib.check_multi(call(_lib.load(), (C.c_int * max(D, 1))(*bits), _ptr(eig) if eig is not None else None, _ptr(cent),
                          _ptr(q)))
    return cent, q


def _lut_fit_quantiles_multi(devices, X, bits, eigvec, u8: bool):
    X = _fit_rows(X, u8)
    n_dev, arr = _device_list(devices)
    fn = "vaqhip_multi_lut_fit_quantiles" + ("_u8" if u8 else "")
    return _fit_quantiles_call(X.shape[1], bits, eigvec, lambda L, b, e, c, q: getattr(L, fn)(
        n_dev, arr, _ptr(X), X.shape[0], X.shape[1], b, e, c, q))


def lut_fit_quantiles_multi(devices: Sequence[int], X, bits: Sequence[int], eigvec: Optional[np.ndarray] = None):
    """vaqhip_multi_lut_fit_quantiles: vaqhip_lut_fit_quantiles's (cent[D, 256], q[D, 257]) bit for bit, with the rows
    of X cut over `devices` as VaqHipMulti.set_codes cuts code rows and dimension d fitted on device d % len(devices);
    no device holds all rows.  A device named several times gives logical shards on that GPU."""
    return _lut_fit_quantiles_multi(devices, X, bits, eigvec, False)


def lut_fit_quantiles_multi_u8(devices: Sequence[int], X, bits: Sequence[int], eigvec: Optional[np.ndarray] = None):
    """lut_fit_quantiles_multi from byte rows (vaqhip_multi_lut_fit_quantiles_u8): every shard uploads its slice as
    n_g x D bytes; the result is lut_fit_quantiles_multi's on X.astype(float32), bit for bit.  Anything but a
    contiguous uint8 n x D array is EINVAL."""
    return _lut_fit_quantiles_multi(devices, X, bits, eigvec, True)


def last_lut_fit_multi_timing() -> dict:
    """Figures of the calling thread's last sharded fit (vaqhip_multi_last_lut_fit_timing)."""
    t = _lib.MultiLutFitTiming()
    _lib.check_multi(_lib.load().vaqhip_multi_last_lut_fit_timing(C.byref(t)))
    return _struct_dict(t)
