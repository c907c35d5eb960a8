"""VaqBitVec: the Hamming half of BitVecEngine (BitVecEngine::query and ::queryRerank with QueryMethod::Sort) over
packed bit rows resident on the device, over vaqhip_bitvec_* of include/vaqhip.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._adapt import _Handle, _dptr, _eig_f32, _f32_rows, _out_pair, _ptr, _stream, _u8_rows, _u8_rows_device


class QueryMethod:
    """BitVecEngine::QueryMethod (BitVecEngine.hpp:82-84).  Only Sort is provided, and for query_naive_ti only Heap
    (include/vaqhip.h says why)."""
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

    The engine can make the bits itself, from raw rows on the host, on the device or in a refiner:

        bv.set_encoder(D, eigvec)                             # binaryEncodingSimple; with bits and thresholds
        bv.encode_from_refiner(r)                             # (bitvec_fit_thresholds): binaryEncoding
        labels, dist = bv.query_device(bv.encode(d_XTest), 100)

    The sub-linear forms visit only the members of the clusters nearest to each query (queryWithClusterInfo):

        bv.set_clusters(centroids, clust_idx)                 # loadCentroids, loadClusterInfo
        bv.set_clusters_from_refiner(centroids, r)            # or with clust_idx made on the device (computeClusterIndex)
        labels, dist = bv.query_clusters(Qbits, XTest, 100, atleast_cluster=8)
        ans = bv.query_rerank_clusters(Qbits, XTest, 100, 10, r, atleast_cluster=8)
        ans = bv.query_naive_clusters(XTest, 100, r, atleast_cluster=8)   # exact distances to every member visited

    The exact search with triangle-inequality pruning (queryNaiveTriangleInequality) has the exhaustive answer:

        bv.set_ti_clusters_from_refiner(centroids, r)         # computeTriangleInequalityClusters
        labels, dist, evaluated = bv.query_naive_ti(XTest, 100, r, evaluated=True)
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

    # ---- the encoders: raw rows -> bit rows on the device ----
    def set_encoder(self, D: int, eigvec=None, bits=None, thresholds=None) -> None:
        """The encoder of the rows and queries to come: BitVecEngine::binaryEncodingSimple (bits None: one sign bit per
        dimension, n_bits == D) or ::binaryEncoding (bits[D] in 0..8, thresholds float32 [D][256] as
        bitvec_fit_thresholds leaves them, n_bits == sum(bits)).  eigvec: D x D, or None for rows already projected."""
        self.enc_D = int(D)
        eig = _eig_f32(eigvec, self.enc_D, "eigvec")
        b = thr = None
        if bits is not None:
            b = (C.c_int * self.enc_D)(*_bits_list(bits, self.enc_D))
            thr = _thresholds(thresholds, self.enc_D)
        self._call("set_encoder", self.enc_D, _ptr(eig) if eig is not None else None, b,
                   _ptr(thr) if thr is not None else None)

    def _raw(self, X):
        """(rows, "_u8" or ""): uint8 rows stay bytes, anything else is taken as float32; n x D of the encoder."""
        D = getattr(self, "enc_D", 0)
        if not D:
            raise _lib.VaqHipError(-7, "no encoder: call set_encoder first")
        if hasattr(X, "data_ptr"):
            import torch
            if X.dtype == torch.uint8:
                return _u8_rows_device(X, D), "_u8"
            if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] == D and X.is_contiguous()):
                raise _lib.VaqHipError(-1, f"device rows must be a contiguous float32 or uint8 n x {D} CUDA tensor")
            return X, ""
        if getattr(X, "dtype", None) == np.uint8:
            return _u8_rows(X, D), "_u8"
        return _f32_rows(X, D, "rows {shape} are not n x {D}"), ""

    def encode(self, X, out=None):
        """The bit rows of raw rows (or of a query batch): a host array gives uint64 [n][W]; a torch CUDA tensor (float32
        or uint8) gives an int64 [n][W] tensor, enqueued on torch's current stream with no synchronisation."""
        X, u8 = self._raw(X)
        if hasattr(X, "data_ptr"):
            import torch
            if X.device.index != self.device:
                raise _lib.VaqHipError(-1, f"device rows must be on cuda:{self.device}")
            if out is None:
                out = torch.empty((X.shape[0], self.W), dtype=torch.int64, device=X.device)
            self._call("encode" + u8 + "_device", _dptr(X), X.shape[0], _dptr(self._words_device(out, "out")), _stream(X))
            return out
        rows = np.empty((X.shape[0], self.W), np.uint64)
        self._call("encode" + u8, _ptr(X), X.shape[0], _ptr(rows))
        return rows

    def set_rows_encoded(self, X, id_base: int = 0) -> None:
        """set_rows(encode(X)) from raw host rows, the bits written straight into the engine's store."""
        X, u8 = self._raw(np.asarray(X))
        self._call("encode_set_rows" + u8, _ptr(X), X.shape[0], int(id_base))

    def add_rows_encoded(self, X) -> None:
        """add_rows(encode(X)) from raw host rows."""
        X, u8 = self._raw(np.asarray(X))
        self._call("encode_add_rows" + u8, _ptr(X), X.shape[0])

    def encode_from_refiner(self, refiner, id_base: int = 0) -> None:
        """Replace the rows by the encoded rows a VaqRefiner on the same device holds (float or byte), read in place."""
        self._call("encode_from_refiner", refiner._h, int(id_base))

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

    # ---- the cluster forms: BitVecEngine::queryWithClusterInfo and ::queryRerankWithClusterInfo ----
    def set_clusters(self, centroids, clust_idx) -> None:
        """loadCentroids and loadClusterInfo: centroids float32 [T][D], clust_idx int32 [n] = the cluster of each row
        held.  Keeps a second, cluster-major copy of the bit rows on the device.  Whatever replaces or appends rows
        drops the state: call this again behind it."""
        cen = np.ascontiguousarray(centroids, dtype=np.float32)
        if cen.ndim != 2 or cen.shape[0] < 1 or cen.shape[1] < 1:
            raise _lib.VaqHipError(-1, f"centroids {cen.shape} are not T x D")
        idx = np.asarray(clust_idx)
        if idx.ndim != 1 or idx.dtype.kind not in "iu":
            raise _lib.VaqHipError(-1, "clust_idx must be a one-dimensional integer array")
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= cen.shape[0]):
            raise _lib.VaqHipError(-1, f"clust_idx outside 0..{cen.shape[0] - 1}")
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.shape[0] != len(self):
            raise _lib.VaqHipError(-1, f"{idx.shape[0]} cluster indices for {len(self)} rows")
        self._call("set_clusters", _ptr(cen), cen.shape[0], cen.shape[1], _ptr(idx))
        self.cluster_D = cen.shape[1]

    def set_clusters_from_refiner(self, centroids, refiner) -> None:
        """set_clusters(centroids, refiner.cluster_index(centroids)) with the assignment made on the device
        (computeClusterIndex over the refiner's rows, float or byte): the refiner holds the raw rows of the bit rows
        held.  A row with no centre below FLT_MAX (index -1) is EINVAL and the state stays as it was."""
        cen = np.ascontiguousarray(centroids, dtype=np.float32)
        if cen.ndim != 2 or cen.shape[0] < 1 or cen.shape[1] < 1:
            raise _lib.VaqHipError(-1, f"centroids {cen.shape} are not T x D")
        self._call("set_clusters_from_refiner", refiner._h, _ptr(cen), cen.shape[0], cen.shape[1])
        self.cluster_D = cen.shape[1]

    def _ori(self, Q, ori_queries) -> np.ndarray:
        D = getattr(self, "cluster_D", 0)
        if not D:
            raise _lib.VaqHipError(-7, "no cluster state: call set_clusters first")
        XQ = _f32_rows(ori_queries, D, "oriQueries {shape} are not nq x {D}")
        if XQ.shape[0] != Q.shape[0]:
            raise _lib.VaqHipError(-1, f"{Q.shape[0]} bit queries but {XQ.shape[0]} original queries")
        return XQ

    def _ori_device(self, q, d_ori_queries):
        import torch
        D = getattr(self, "cluster_D", 0)
        if not D:
            raise _lib.VaqHipError(-7, "no cluster state: call set_clusters first")
        oq = d_ori_queries.contiguous()
        if not (oq.is_cuda and oq.device == q.device and oq.dtype == torch.float32 and tuple(oq.shape) == (q.shape[0], D)):
            raise _lib.VaqHipError(-1, f"device oriQueries must be float32 {q.shape[0]} x {D} on the queries' device")
        return oq

    def query_clusters(self, queries, ori_queries, k: int, method: int = QueryMethod.Sort, atleast_cluster: int = 1):
        """BitVecEngine::queryWithClusterInfo: the k best among the members of the clusters nearest to each original
        query (as many as hold k rows, and atleast_cluster at least): (labels int32 [nq][k], distances uint32
        [nq][k]), slots past the candidates -1 / 0xffffffff."""
        Q = self._words(queries, "queries")
        XQ = self._ori(Q, ori_queries)
        nq = Q.shape[0]
        lab = np.empty((nq, k), np.int32)
        dis = np.empty((nq, k), np.float32)
        self._call("query_clusters", _ptr(Q), _ptr(XQ), nq, int(k), int(method), int(atleast_cluster), _ptr(lab), _ptr(dis))
        out = np.full((nq, k), 0xffffffff, np.uint32)
        np.copyto(out, dis, where=lab >= 0, casting="unsafe")
        return lab, out

    def query_clusters_device(self, d_queries, d_ori_queries, k: int, method: int = QueryMethod.Sort,
                              atleast_cluster: int = 1, out=None):
        """query_clusters() on torch CUDA tensors, enqueued on torch's current stream, no synchronisation: distances
        float32, the exact integers; empty slots -1 / FLT_MAX."""
        q = self._words_device(d_queries, "device queries")
        oq = self._ori_device(q, d_ori_queries)
        nq = q.shape[0]
        labels, dists = _out_pair(out, nq, k, q.device)
        self._call("query_clusters_device", _dptr(q), _dptr(oq), nq, int(k), int(method), int(atleast_cluster),
                   _dptr(labels), _dptr(dists), _stream(q))
        return labels, dists

    def query_rerank_clusters(self, queries, ori_queries, k: int, factor: int, refiner, atleast_cluster: int = 1):
        """BitVecEngine::queryRerankWithClusterInfo: query_clusters with min(factor * k, n) candidates, reranked as
        query_rerank does: (labels int32 [nq][k], squared Euclidean distances float32 [nq][k])."""
        Q = self._words(queries, "queries")
        XQ = self._ori(Q, ori_queries)
        nq = Q.shape[0]
        lab = np.empty((nq, k), np.int32)
        dis = np.empty((nq, k), np.float32)
        self._call("query_rerank_clusters", refiner._h, _ptr(Q), _ptr(XQ), nq, int(k), int(factor), int(atleast_cluster),
                   _ptr(lab), _ptr(dis))
        return lab, dis

    def query_rerank_clusters_device(self, d_queries, d_ori_queries, k: int, factor: int, refiner,
                                     atleast_cluster: int = 1, out=None):
        """query_rerank_clusters() on torch CUDA tensors, enqueued on torch's current stream, no synchronisation."""
        q = self._words_device(d_queries, "device queries")
        oq = self._ori_device(q, d_ori_queries)
        nq = q.shape[0]
        labels, dists = _out_pair(out, nq, k, q.device)
        self._call("query_rerank_clusters_device", refiner._h, _dptr(q), _dptr(oq), nq, int(k), int(factor),
                   int(atleast_cluster), _dptr(labels), _dptr(dists), _stream(q))
        return labels, dists

    # ---- the exact cluster form: BitVecEngine::queryNaiveWithClusterInfo ----
    def query_naive_clusters(self, ori_queries, k: int, refiner, method: int = QueryMethod.Sort, atleast_cluster: int = 1):
        """BitVecEngine::queryNaiveWithClusterInfo: the k best by exact squared Euclidean distance among ALL members of
        the clusters query_clusters would visit, over the rows of a VaqRefiner on the same device (float or byte); no
        bits are read.  (labels int32 [nq][k], distances float32 [nq][k]); slots past the candidates -1 / FLT_MAX."""
        D = getattr(self, "cluster_D", 0)
        if not D:
            raise _lib.VaqHipError(-7, "no cluster state: call set_clusters first")
        XQ = _f32_rows(ori_queries, D, "oriQueries {shape} are not nq x {D}")
        nq = XQ.shape[0]
        lab = np.empty((nq, k), np.int32)
        dis = np.empty((nq, k), np.float32)
        self._call("query_naive_clusters", refiner._h, _ptr(XQ), nq, int(k), int(method), int(atleast_cluster), _ptr(lab),
                   _ptr(dis))
        return lab, dis

    def query_naive_clusters_device(self, d_ori_queries, k: int, refiner, method: int = QueryMethod.Sort,
                                    atleast_cluster: int = 1, out=None):
        """query_naive_clusters() on a float32 [nq][D] torch CUDA tensor, enqueued on torch's current stream, no
        synchronisation."""
        import torch
        D = getattr(self, "cluster_D", 0)
        if not D:
            raise _lib.VaqHipError(-7, "no cluster state: call set_clusters first")
        oq = d_ori_queries.contiguous()
        if not (oq.is_cuda and oq.device.index == self.device and oq.dtype == torch.float32 and oq.dim() == 2 and oq.shape[1] == D):
            raise _lib.VaqHipError(-1, f"device oriQueries must be float32 nq x {D} on cuda:{self.device}")
        nq = oq.shape[0]
        labels, dists = _out_pair(out, nq, k, oq.device)
        self._call("query_naive_clusters_device", refiner._h, _dptr(oq), nq, int(k), int(method), int(atleast_cluster),
                   _dptr(labels), _dptr(dists), _stream(oq))
        return labels, dists

    # ---- the triangle-inequality form: BitVecEngine::queryNaiveTriangleInequality ----
    def set_ti_clusters_from_refiner(self, centroids, refiner) -> None:
        """computeTriangleInequalityClusters on the device: every row of the refiner (float or byte) gets its nearest
        centre as set_clusters_from_refiner gives it, and the rows are grouped cluster after cluster, the farthest from its
        centre first.  The raw rows stay in the refiner.  Separate from set_clusters' state; dropped with it."""
        cen = np.ascontiguousarray(centroids, dtype=np.float32)
        if cen.ndim != 2 or cen.shape[0] < 1 or cen.shape[1] < 1:
            raise _lib.VaqHipError(-1, f"centroids {cen.shape} are not T x D")
        self._call("set_ti_clusters_from_refiner", refiner._h, _ptr(cen), cen.shape[0], cen.shape[1])

    def query_naive_ti(self, ori_queries, k: int, refiner, method: int = QueryMethod.Heap, evaluated: bool = False):
        """BitVecEngine::queryNaiveTriangleInequality: the k nearest of ALL rows by (Euclidean distance, label), exact; the
        rows a centre distance proves out of reach are never loaded.  (labels int32 [nq][k], distances float32 [nq][k], the
        square roots); slots past min(k, n) are -1 / FLT_MAX.  evaluated=True adds int64 [nq], the rows each query loaded.
        Before set_ti_clusters_from_refiner, or once the rows have changed, the call is VAQHIP_ESTATE."""
        XQ = _f32_rows(ori_queries, refiner.D, "oriQueries {shape} are not nq x {D}")
        nq = XQ.shape[0]
        lab = np.empty((nq, k), np.int32)
        dis = np.empty((nq, k), np.float32)
        ev = np.zeros(nq, np.int64) if evaluated else None
        self._call("query_naive_ti", refiner._h, _ptr(XQ), nq, int(k), int(method), _ptr(lab), _ptr(dis),
                   _ptr(ev) if evaluated else None)
        return (lab, dis, ev) if evaluated else (lab, dis)

    def query_naive_ti_device(self, d_ori_queries, k: int, refiner, method: int = QueryMethod.Heap, out=None,
                              evaluated_out=None):
        """query_naive_ti() on a float32 [nq][D] torch CUDA tensor, enqueued on torch's current stream, no
        synchronisation.  evaluated_out: an int64 [nq] tensor on the same device, or None."""
        import torch
        D = refiner.D
        oq = d_ori_queries.contiguous()
        if not (oq.is_cuda and oq.device.index == self.device and oq.dtype == torch.float32 and oq.dim() == 2 and oq.shape[1] == D):
            raise _lib.VaqHipError(-1, f"device oriQueries must be float32 nq x {D} on cuda:{self.device}")
        nq = oq.shape[0]
        ev = evaluated_out
        if ev is not None and not (ev.is_cuda and ev.device == oq.device and ev.dtype == torch.int64 and ev.is_contiguous()
                                   and tuple(ev.shape) == (nq,)):
            raise _lib.VaqHipError(-1, f"evaluated_out must be a contiguous int64 [{nq}] tensor on the queries' device")
        labels, dists = _out_pair(out, nq, k, oq.device)
        self._call("query_naive_ti_device", refiner._h, _dptr(oq), nq, int(k), int(method), _dptr(labels), _dptr(dists),
                   _dptr(ev) if ev is not None else None, _stream(oq))
        return labels, dists


def _bits_list(bits, D: int):
    b = [int(x) for x in bits]
    if len(b) != D:
        raise _lib.VaqHipError(-1, f"{len(b)} bit counts for D={D}")
    return b


def _thresholds(thr, D: int) -> np.ndarray:
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    if thr.shape != (D, 256):
        raise _lib.VaqHipError(-1, f"thresholds {thr.shape} are not {D} x 256")
    return thr


def _fit_thresholds(X, bits, eigvec, device: int, u8: bool, out):
    if hasattr(X, "data_ptr"):
        import torch
        X = _u8_rows_device(X, X.shape[-1]) if u8 else X
        if not (X.is_cuda and X.dim() == 2 and X.is_contiguous() and X.dtype == (torch.uint8 if u8 else torch.float32)):
            raise _lib.VaqHipError(-1, "device rows must be a contiguous n x D CUDA tensor of the call's element type")
        n, D = X.shape
        if eigvec is not None and not (eigvec.is_cuda and eigvec.dtype == torch.float32 and tuple(eigvec.shape) == (D, D)
                                       and eigvec.is_contiguous()):
            raise _lib.VaqHipError(-1, f"device eigvec must be a contiguous float32 {D} x {D} CUDA tensor")
        if out is None:
            out = torch.zeros((D, 256), dtype=torch.float32, device=X.device)
        b = (C.c_int * D)(*_bits_list(bits, D))
        fn = getattr(_lib.load(), "vaqhip_bitvec_fit_thresholds" + ("_u8" if u8 else "") + "_device")
        _lib.check(fn(X.device.index, _dptr(X), n, D, b, _dptr(eigvec) if eigvec is not None else None, _dptr(out), _stream(X)))
        return out
    X = np.asarray(X)
    X = _u8_rows(X, X.shape[-1]) if u8 else _f32_rows(X, X.shape[-1], "rows {shape} are not n x {D}")
    n, D = X.shape
    eig = _eig_f32(eigvec, D, "eigvec")
    out = np.zeros((D, 256), np.float32) if out is None else _thresholds(out, D)
    b = (C.c_int * D)(*_bits_list(bits, D))
    fn = getattr(_lib.load(), "vaqhip_bitvec_fit_thresholds" + ("_u8" if u8 else ""))
    _lib.check(fn(device, _ptr(X), n, D, b, _ptr(eig) if eig is not None else None, _ptr(out)))
    return out


def bitvec_fit_thresholds(X, bits, eigvec=None, device: int = 0, out=None):
    """The quantile thresholds of BitVecEngine::binaryEncoding from raw float rows: float32 [D][256], row d holding its
    2^bits[d] entries (the last is FLT_MAX); the rest of `out` (zeros when it is not given) is left as it is.  Host
    arrays, or torch CUDA tensors (X, eigvec, out), on whose device and current stream the fit then runs."""
    return _fit_thresholds(X, bits, eigvec, device, False, out)


def bitvec_fit_thresholds_u8(X, bits, eigvec=None, device: int = 0, out=None):
    """bitvec_fit_thresholds from byte rows (a bvecs dataset as its file holds it)."""
    return _fit_thresholds(X, bits, eigvec, device, True, out)
