"""VaqBitVec: the Hamming half of BitVecEngine (BitVecEngine::query and ::queryRerank with QueryMethod::Sort) over
packed bit rows resident on the device, over vaqhip_bitvec_* of include/vaqhip.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._adapt import _Handle, _dptr, _f32_rows, _out_pair, _ptr, _stream


class QueryMethod:
    """BitVecEngine::QueryMethod (BitVecEngine.hpp:82-84).  Only Sort is provided (include/vaqhip.h says why)."""
    Heap = 0
    Sort = 1
    HeapEarlyAbandon = 2
    SortEarlyAbandon = 3


class VaqBitVec(_Handle):
    """BitVecEngine's bit vectors on the GPU: rows of W = (n_bits + 63) // 64 uint64 words, as `bitv` holds them (no
    masking: whatever the tail bits of the last word hold counts).  The answers are the reference's slot for slot,
    equal distances included (KNNFromDists / KNNFromDistsIndicesSupplied).

        bv = VaqBitVec(device=0, n_bits=128)
        bv.set_rows(harness.sign_bits(XTrainPCA))            # uint64 [n][W]
        labels, dist = bv.query(harness.sign_bits(XTestPCA), 100)
        r = VaqRefiner(D); r.set_rows_u8(XTrain)              # originalData
        ans = bv.query_rerank(Qbits, XTest, 100, 10, r)       # queryRerank(..., k, factor)
    """
    _destroy = "vaqhip_bitvec_destroy"

    def __init__(self, device: int = 0, n_bits: int = 64):
        self.device = device
        self.n_bits = int(n_bits)
        self.W = (self.n_bits + 63) // 64
        self._h = C.c_void_p()
        h = C.c_void_p()
        _lib.check(_lib.load().vaqhip_bitvec_create(C.byref(h), device, self.n_bits))
        self._h = h

    def _call(self, name: str, *args) -> int:
        return _lib.check(getattr(_lib.load(), "vaqhip_bitvec_" + name)(self._h, *args))

    def _words(self, X, what: str) -> np.ndarray:
        """Bit rows as the calls take them: a contiguous uint64 n x W array; nothing is converted."""
        X = np.asarray(X)
        if X.dtype != np.uint64 or X.ndim != 2 or X.shape[1] != self.W or not X.flags.c_contiguous:
            raise _lib.VaqHipError(-1, f"{what} must be a contiguous uint64 n x {self.W} array (nothing is converted)")
        return X

    def _words_device(self, t, what: str):
        """The same for a torch CUDA tensor: int64 (torch has no unsigned 64-bit arithmetic; the bits are the same)."""
        import torch
        if not (t.is_cuda and t.device.index == self.device and t.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
                and t.dim() == 2 and t.shape[1] == self.W and t.is_contiguous()):
            raise _lib.VaqHipError(-1, f"{what} must be a contiguous 64-bit integer n x {self.W} tensor on cuda:{self.device}")
        return t

    def set_rows(self, rows, id_base: int = 0) -> None:
        """Replace the rows: a uint64 [n][W] host array, or a 64-bit integer torch tensor on the engine's device
        (copied).  Row i has label id_base + i."""
        if hasattr(rows, "data_ptr"):
            t = self._words_device(rows, "device rows")
            self._call("set_rows_device", _dptr(t), t.shape[0], int(id_base), _stream(t))
            return
        X = self._words(rows, "rows")
        self._call("set_rows", _ptr(X), X.shape[0], int(id_base))

    def add_rows(self, rows) -> None:
        """Append rows; their labels continue behind the rows already held."""
        X = self._words(rows, "rows")
        self._call("add_rows", _ptr(X), X.shape[0])

    def __len__(self) -> int:
        return int(self._call("size"))

    def set_option(self, key: str, value: int) -> None:
        """"dist_chunk_bytes": the bound on the distance matrix of one chunk of queries (default 2^30)."""
        self._call("set_option", key.encode(), int(value))

    def query(self, queries, k: int, method: int = QueryMethod.Sort):
        """BitVecEngine::query: (labels int32 [nq][k], distances uint32 [nq][k]).  Slots past min(k, n) hold label -1 and
        distance 0xffffffff."""
        Q = self._words(queries, "queries")
        nq = Q.shape[0]
        lab = np.empty((nq, k), np.int32)
        dis = np.empty((nq, k), np.float32)
        self._call("query", _ptr(Q), nq, int(k), int(method), _ptr(lab), _ptr(dis))
        out = np.full((nq, k), 0xffffffff, np.uint32)
        np.copyto(out, dis, where=lab >= 0, casting="unsafe")
        return lab, out

    def query_device(self, d_queries, k: int, method: int = QueryMethod.Sort, out=None):
        """query() on torch CUDA tensors, enqueued on torch's current stream, no synchronisation: (labels int32 [nq][k],
        distances float32 [nq][k], the exact integers; slots past min(k, n) are -1 / FLT_MAX)."""
        q = self._words_device(d_queries, "device queries")
        nq = q.shape[0]
        labels, dists = _out_pair(out, nq, k, q.device)
        self._call("query_device", _dptr(q), nq, int(k), int(method), _dptr(labels), _dptr(dists), _stream(q))
        return labels, dists

    def query_rerank(self, queries, ori_queries, k: int, factor: int, refiner):
        """BitVecEngine::queryRerank(queries, oriQueries, k, factor) over the rows of a VaqRefiner on the same device
        (originalData, float or byte): (labels int32 [nq][k], squared Euclidean distances float32 [nq][k]); slots past
        min(k, factor * k, n) are -1 / FLT_MAX."""
        Q = self._words(queries, "queries")
        XQ = _f32_rows(ori_queries, refiner.D, "oriQueries {shape} are not nq x {D}")
        nq = Q.shape[0]
        if XQ.shape[0] != nq:
            raise _lib.VaqHipError(-1, f"{nq} bit queries but {XQ.shape[0]} original queries")
        lab = np.empty((nq, k), np.int32)
        dis = np.empty((nq, k), np.float32)
        self._call("query_rerank", refiner._h, _ptr(Q), _ptr(XQ), nq, int(k), int(factor), _ptr(lab), _ptr(dis))
        return lab, dis

    def query_rerank_device(self, d_queries, d_ori_queries, k: int, factor: int, refiner, out=None):
        """query_rerank() on torch CUDA tensors, enqueued on torch's current stream, no synchronisation."""
        import torch
        q = self._words_device(d_queries, "device queries")
        oq = d_ori_queries.contiguous()
        if not (oq.is_cuda and oq.dtype == torch.float32 and oq.dim() == 2 and oq.shape == (q.shape[0], refiner.D)):
            raise _lib.VaqHipError(-1, f"device oriQueries must be float32 {q.shape[0]} x {refiner.D}")
        nq = q.shape[0]
        labels, dists = _out_pair(out, nq, k, q.device)
        self._call("query_rerank_device", refiner._h, _dptr(q), _dptr(oq), nq, int(k), int(factor), _dptr(labels),
                   _dptr(dists), _stream(q))
        return labels, dists
