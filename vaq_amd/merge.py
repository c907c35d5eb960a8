"""The exchange step of a multi-GPU search as free functions over torch CUDA tensors (vaqhip_merge_*_device):
per-shard top-k lists in, one merged (labels, distances) pair out, enqueued on torch's current stream."""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._adapt import _dptr, _out_pair, _stream


def _merge_call(t, nq: int, k: int, out, call):
    """What the three merges share: the output pair, the device and stream of tensor t, the check.
    call(device, out_labels, out_dists, stream) -> code."""
    import torch
    out_l, out_d = _out_pair(out, nq, k, t.device)
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    _lib.check(call(dev, _dptr(out_l), _dptr(out_d), _stream(t)))
    return out_l, out_d


def _lists(dist_lists, label_lists, k: int):
    import torch
    d = dist_lists.contiguous()
    l = label_lists.contiguous()
    n_lists, nq, kk = d.shape
    assert kk == k and l.shape == d.shape and l.dtype == torch.int32 and d.dtype == torch.float32
    return d, l, n_lists, nq


def merge_topk_device(dist_lists, label_lists, k: int, out=None):
    """Multi-GPU exchange step: [n_lists, nq, k] CUDA tensors (labels global,
    empty slots -1 / FLT_MAX) -> per-query k smallest by (distance, label)."""
    d, l, n_lists, nq = _lists(dist_lists, label_lists, k)
    return _merge_call(d, nq, k, out, lambda dev, out_l, out_d, st: _lib.load().vaqhip_merge_topk_device(
        dev, _dptr(d), _dptr(l), n_lists, nq, k, out_l, out_d, st))


def merge_topk_packed_device(packed, world: int, nq: int, k: int, out=None):
    """packed: int32 CUDA tensor [world, 2, nq, k] from ONE all-gather -- plane 0 holds
    labels, plane 1 the float32 distance bits.  Returns the merged (labels, distances)."""
    import torch
    assert packed.is_contiguous() and packed.dtype == torch.int32 and packed.numel() == world * 2 * nq * k
    base = packed.data_ptr()
    return _merge_call(packed, nq, k, out, lambda dev, out_l, out_d, st: _lib.load().vaqhip_merge_topk_strided_device(
        dev, C.c_void_p(base + nq * k * 4), C.c_void_p(base), world, 2 * nq * k, k, nq, k, out_l, out_d, st))


def merge_fast_device(head_dist, dist_lists, label_lists, k: int, head_label_base: int = 0, out=None):
    """FAST's exchange step (vaqhip_merge_fast_device): head_dist uint16-valued int16 CUDA tensor [nq, n_head]
    -- the distances of the first n_head = min(k, N) rows of the whole database -- and [n_lists, nq, k] lists of
    the OTHER rows, each ascending by (distance, row), lists in row order, empty slots -1 / FLT_MAX.  Returns the
    single index's FAST answer: the first k of the stable merge by distance of the head in std::sort's order,
    then the lists."""
    d, l, n_lists, nq = _lists(dist_lists, label_lists, k)
    h = head_dist.contiguous()
    assert h.dim() == 2 and h.shape[0] == nq and h.element_size() == 2 and h.shape[1] <= k
    return _merge_call(d, nq, k, out, lambda dev, out_l, out_d, st: _lib.load().vaqhip_merge_fast_device(
        dev, _dptr(h), h.shape[1], h.shape[1], int(head_label_base), _dptr(d), _dptr(l), n_lists, nq * k, k, nq, k,
        out_l, out_d, st))
