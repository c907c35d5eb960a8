"""cluster_index: the cluster of every raw row (computeClusterIndex) made on the device, over vaqhip_cluster_index* and
vaqhip_refiner_cluster_index* of include/vaqhip.h -- what VaqBitVec.set_clusters takes as clust_idx."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._adapt import _dptr, _f32_rows, _ptr, _stream, _u8_rows, _u8_rows_device


def _centres(centroids) -> np.ndarray:
    cen = np.ascontiguousarray(centroids, dtype=np.float32)
    if cen.ndim != 2 or cen.shape[0] < 1 or cen.shape[1] < 1:
        raise _lib.VaqHipError(-1, f"centroids {cen.shape} are not T x D")
    return cen


def _centres_device(d_centroids, device, D: int):
    import torch
    c = d_centroids.contiguous()
    if not (c.is_cuda and c.device == device and c.dtype == torch.float32 and c.dim() == 2 and c.shape[0] >= 1 and c.shape[1] == D):
        raise _lib.VaqHipError(-1, f"device centroids must be float32 T x {D} on {device}")
    return c


def _outputs(n: int, return_dist: bool):
    return np.empty(n, np.int32), (np.empty(n, np.float32) if return_dist else None)


def _outputs_device(n: int, return_dist: bool, device):
    import torch
    return (torch.empty(n, dtype=torch.int32, device=device),
            torch.empty(n, dtype=torch.float32, device=device) if return_dist else None)


def _cluster_index(X, centroids, device: int, return_dist: bool, u8: bool):
    name = "vaqhip_cluster_index" + ("_u8" if u8 else "")
    if hasattr(X, "data_ptr"):
        import torch
        if not (X.is_cuda and X.dim() == 2 and X.is_contiguous() and X.dtype == (torch.uint8 if u8 else torch.float32)):
            raise _lib.VaqHipError(-1, "device rows must be a contiguous n x D CUDA tensor of the call's element type")
        X = _u8_rows_device(X, X.shape[1]) if u8 else X
        n, D = X.shape
        cen = _centres_device(centroids, X.device, D)
        idx, dist = _outputs_device(n, return_dist, X.device)
        _lib.check(getattr(_lib.load(), name + "_device")(X.device.index, _dptr(X), n, D, _dptr(cen), cen.shape[0], _dptr(idx),
                                                          _dptr(dist) if return_dist else None, _stream(X)))
        return (idx, dist) if return_dist else idx
    cen = _centres(centroids)
    X = _u8_rows(X, cen.shape[1]) if u8 else _f32_rows(X, cen.shape[1], "rows {shape} are not n x {D}")
    n, D = X.shape
    idx, dist = _outputs(n, return_dist)
    _lib.check(getattr(_lib.load(), name)(int(device), _ptr(X), n, D, _ptr(cen), cen.shape[0], _ptr(idx),
                                          _ptr(dist) if return_dist else None))
    return (idx, dist) if return_dist else idx


def cluster_index(X, centroids, device: int = 0, return_dist: bool = False):
    """computeClusterIndex: int32 [n], the first nearest of the T centres (float32 [T][D]) for every row of X (float32
    [n][D]) by one float accumulator in dimension order; -1 where no distance is below FLT_MAX (a NaN, an overflow).
    return_dist: also the chosen centre's squared distance, float32 [n].  Host arrays (staged through `device` in
    pieces), or torch CUDA tensors (X and centroids), on whose device and current stream the kernel is enqueued."""
    return _cluster_index(X, centroids, device, return_dist, False)


def cluster_index_u8(X, centroids, device: int = 0, return_dist: bool = False):
    """cluster_index from byte rows (a bvecs dataset as its file holds it): the answer over X.astype(float32)."""
    return _cluster_index(X, centroids, device, return_dist, True)
