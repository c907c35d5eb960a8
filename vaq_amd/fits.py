"""The fits that need no index: the subspace codebooks (vaqhip_fit_codebooks*, vaqhip_multi_fit_codebooks*) and
binaryEncodingLUT's quantile codebooks over several devices (vaqhip_multi_lut_fit_quantiles*), with their timing
calls.  The byte-row form of a fit is the float form's body with the other symbol."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._adapt import _dptr, _eig_f32, _ptr, _stream, _struct_dict, _u8_rows


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


def _fit_codebooks_form(form: str, X, M, bits, eigvec, max_iter, device, u8: bool):
    """A wide form of the fit ("hier" or "bin"): vaqhip_fit_codebooks_<form>[_u8]."""
    X = _fit_rows(X, u8)
    fn = "vaqhip_fit_codebooks_" + form + ("_u8" if u8 else "")
    return _fit_codebooks_call(X.shape[1], M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: getattr(L, fn)(
        int(device), _ptr(X), X.shape[0], X.shape[1], int(M), b, e, it, c, i, nn))


def fit_codebooks_hier(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25,
                       device: int = 0):
    """vaqhip_fit_codebooks_hier: fit_codebooks with every subspace above 8 bits fitted in two stages, as VAQ::train
    does under mHierarchicalKmeans (demo_vaq --kmeans-ver 1): 128 centres over the head of randomPermutation(n), the
    rows split by nearest centre (squaredNorm, no sqrt), then 1 << (bits - 7) centres inside each group.  Subspaces of
    at most 8 bits, and a call without any wider one, are fit_codebooks's bit for bit.  Returns what fit_codebooks
    returns; iterations[s] is the largest count among a hierarchical subspace's 129 fits.  Single device only."""
    return _fit_codebooks_form("hier", X, M, bits, eigvec, max_iter, device, False)


def fit_codebooks_hier_u8(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25,
                          device: int = 0):
    """fit_codebooks_hier from byte rows (vaqhip_fit_codebooks_hier_u8): its result on X.astype(float32), bit for bit."""
    return _fit_codebooks_form("hier", X, M, bits, eigvec, max_iter, device, True)


def last_fit_codebooks_hier_timing() -> dict:
    """Figures of the calling thread's last hierarchical fit (vaqhip_last_fit_codebooks_hier_timing): stage1_ms,
    regroup_ms, stage2_ms, the groups and the smallest and largest of them, the iterations per stage."""
    t = _lib.FitCodebooksHierTiming()
    _lib.check(_lib.load().vaqhip_last_fit_codebooks_hier_timing(C.byref(t)))
    return _struct_dict(t)


def fit_codebooks_bin(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25,
                      device: int = 0):
    """vaqhip_fit_codebooks_bin: fit_codebooks with every subspace above 8 bits fitted as a binary tree, as VAQ::train
    does under mBinaryKmeans (demo_vaq --kmeans-ver 2): a 2-centre fit per node, the node's rows split by the nearer
    centre (squaredNorm, no sqrt, ties right), down to depth bits[s]; a node whose split leaves a side with fewer rows
    than it needs centres is fitted flat and ends its branch.  No group size is refused: the form for skewed data.
    Subspaces of at most 8 bits, and a call without any wider one, are fit_codebooks's bit for bit.  Returns what
    fit_codebooks returns; iterations[s] is the largest count among a binary subspace's fits.  Single device only."""
    return _fit_codebooks_form("bin", X, M, bits, eigvec, max_iter, device, False)


def fit_codebooks_bin_u8(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25,
                         device: int = 0):
    """fit_codebooks_bin from byte rows (vaqhip_fit_codebooks_bin_u8): its result on X.astype(float32), bit for bit."""
    return _fit_codebooks_form("bin", X, M, bits, eigvec, max_iter, device, True)


def last_fit_codebooks_bin_timing() -> dict:
    """Figures of the calling thread's last binary fit (vaqhip_last_fit_codebooks_bin_timing): fit_ms, split_ms, cut_ms,
    the levels walked, the 2-centre fits run, the cut and leaf nodes, the fits that sampled."""
    t = _lib.FitCodebooksBinTiming()
    _lib.check(_lib.load().vaqhip_last_fit_codebooks_bin_timing(C.byref(t)))
    return _struct_dict(t)


def fit_codebooks_bin_sums(mode: int) -> None:
    """Which kernel adds the binary fit's ordered sums for the calling thread (vaqhip_fit_codebooks_bin_set_sums): 0 the
    staged one (default), 1 the flat fit's; the centres are the same bit for bit."""
    _lib.check(_lib.load().vaqhip_fit_codebooks_bin_set_sums(int(mode)))


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


def _train_rotation_call(D: int, M: int, call):
    """The arrays around a vaqhip_*train_rotation call: (eigvec D x D float32, eigenvalues[D], bits[highest_subs],
    highest_subs).  call(L, eigvec, eigenvalues, bits, highest) with eigvec None: the caller passes its own."""
    M = int(M)
    eig = np.empty((max(D, 1), max(D, 1)), np.float32)
    ev = np.empty(max(D, 1), np.float32)
    bits = np.zeros(max(M, 1), np.int32)
    hi = C.c_int(0)
    _lib.check(call(_lib.load(), _ptr(eig), _ptr(ev), _ptr(bits), C.byref(hi)))
    return eig, ev, [int(b) for b in bits[:hi.value]], hi.value


def train_rotation(X, M: int, bit_budget: int, min_bits: int, max_bits: int, percent_var: float = 1.0, device: int = 0):
    """vaqhip_train_rotation*: the front half of VAQ::train from raw rows -- the second moment of the sampled rows
    (in double, in a fixed order), its eigen-decomposition (Jacobi, on the device), the partial balance and the exact
    bit allocation.  X: n x D rows, a host array (uint8 stays bytes, anything else becomes float32) or a contiguous
    float32 / uint8 torch tensor on the device.  Returns (eigvec float32 D x D with its columns in balanced order,
    eigenvalues[D] in that order, bits[highest_subs], highest_subs): eigvec and bits are what fit_codebooks and
    VaqHip take.  With percent_var < 1 highest_subs may be below M or a subspace may get 0 bits: see train()."""
    if hasattr(X, "data_ptr"):
        import torch
        if not (X.is_cuda and X.dim() == 2 and X.is_contiguous() and X.dtype in (torch.float32, torch.uint8)):
            raise _lib.VaqHipError(-1, "device rows must be a contiguous float32 or uint8 n x D CUDA tensor")
        n, D = (int(v) for v in X.shape)
        fn = "vaqhip_train_rotation_u8_device" if X.dtype == torch.uint8 else "vaqhip_train_rotation_device"
        d_eig = torch.empty((D, D), dtype=torch.float32, device=X.device)
        _, ev, bits, hi = _train_rotation_call(D, M, lambda L, e, v, b, h: getattr(L, fn)(
            X.device.index, _dptr(X), n, D, int(M), int(bit_budget), int(min_bits), int(max_bits), float(percent_var),
            _dptr(d_eig), v, b, h, _stream(X)))
        return d_eig.cpu().numpy(), ev, bits, hi
    u8 = isinstance(X, np.ndarray) and X.dtype == np.uint8
    X = _fit_rows(X, u8)
    fn = "vaqhip_train_rotation" + ("_u8" if u8 else "")
    return _train_rotation_call(X.shape[1], M, lambda L, e, v, b, h: getattr(L, fn)(
        int(device), _ptr(X), X.shape[0], X.shape[1], int(M), int(bit_budget), int(min_bits), int(max_bits),
        float(percent_var), e, v, b, h))


def _check_fittable(M: int, bits, highest: int) -> None:
    """What the chained forms refuse: fit_codebooks takes 1..15 bits over all M subspaces."""
    if highest < int(M) or any(b < 1 for b in bits):
        raise _lib.VaqHipError(-2, f"the allocation {list(bits)} over {highest} of {M} subspaces cannot be fitted: "
                                   "fit_codebooks takes at least 1 bit in every subspace (percent_var < 1)")


def train(X, M: int, bit_budget: int, min_bits: int, max_bits: int, percent_var: float = 1.0, device: int = 0,
          max_iter: int = 25):
    """train_rotation() followed by fit_codebooks() with its eigvec and bits, from host rows: (eigvec, bits,
    centroids [M arrays (1 << bits[s]) x L]) -- an index from raw rows and a bit budget alone.  EUNSUPPORTED (-2)
    where percent_var < 1 leaves highest_subs < M or a subspace without bits."""
    if hasattr(X, "data_ptr"):
        raise _lib.VaqHipError(-2, "train() chains fit_codebooks, which takes host rows: pass a host array, keep the rows "
                                   "in a VaqRefiner and call its train(), or call train_rotation() on the tensor")
    eig, _, bits, hi = train_rotation(X, M, bit_budget, min_bits, max_bits, percent_var, device)
    _check_fittable(M, bits, hi)
    u8 = isinstance(X, np.ndarray) and X.dtype == np.uint8
    cents, _, _ = _fit_codebooks(X, M, bits, eig, max_iter, device, None, u8)
    return eig, bits, cents


def last_train_timing() -> dict:
    """Figures of the calling thread's last train_rotation (vaqhip_last_train_timing)."""
    t = _lib.TrainTiming()
    _lib.check(_lib.load().vaqhip_last_train_timing(C.byref(t)))
    return _struct_dict(t)


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
