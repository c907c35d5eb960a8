"""VaqHipMulti: one index with its rows sharded over several GPUs, over vaqhip_multi_*."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._adapt import _Handle, _dptr, _f32_rows, _out_pair, _ptr, _stream, _struct_dict, _u8_rows
from .single import LabelDistVec, _new_answer


class VaqHipMulti(_Handle):
    """One process, several GPUs (include/vaqhip.h "multi-device"): the rows are sharded
    contiguously over `devices`, every device answers all queries on its shard, one RCCL
    all-gather + merge finishes the search.  Naming a device several times gives logical shards
    on that GPU (gather by device copies) -- the form a one-GPU box can test."""
    _destroy = "vaqhip_multi_destroy"

    def __init__(self, devices: Sequence[int], bits: Sequence[int], cents: Sequence[np.ndarray],
                 eig: Optional[np.ndarray] = None, sequential_sum: bool = False):
        L = _lib.load()
        M = len(bits)
        self._cents = [np.ascontiguousarray(c, dtype=np.float32) for c in cents]
        D = sum(c.shape[1] for c in self._cents)
        self._eig = None if eig is None else np.ascontiguousarray(np.real(eig), dtype=np.float32)
        arr = (C.POINTER(C.c_float) * M)()
        for i, c in enumerate(self._cents):
            arr[i] = c.ctypes.data_as(C.POINTER(C.c_float))
        devs = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        self.D, self.M = D, M
        _lib.check_multi(L.vaqhip_multi_create(C.byref(self._h), D, M, (C.c_int * M)(*bits), arr,
                                               _ptr(self._eig) if self._eig is not None else None,
                                               len(devices), devs, 1 if sequential_sum else 0))

    def set_codes(self, codes: np.ndarray, id_base: int = 0) -> None:
        cb = np.ascontiguousarray(codes, dtype=np.uint16)
        assert cb.ndim == 2 and cb.shape[1] == self.M
        _lib.check_multi(_lib.load().vaqhip_multi_set_codes_u16(self._h, _ptr(cb), cb.shape[0], id_base))

    def add_codes(self, codes: np.ndarray) -> None:
        cb = np.ascontiguousarray(codes, dtype=np.uint16)
        _lib.check_multi(_lib.load().vaqhip_multi_add_codes_u16(self._h, _ptr(cb), cb.shape[0]))

    def _train_rows(self, X) -> np.ndarray:
        return _f32_rows(X, self.D, "rows {shape} are not n x {D}")

    def encode(self, X, projected: bool = True, id_base: int = 0, return_codes: bool = False):
        """vaqhip_multi_encode_set_codes: VAQ::encode with every shard encoding the rows it will hold on its own
        device -- the state VaqHip.encode on one index followed by set_codes(codes, id_base) leaves, bit for bit,
        without the codes crossing to the host and back.  projected = False applies the eigenvectors first.
        return_codes: the N x M uint16 matrix VaqHip.encode would have filled (else None)."""
        return self._encode_set(_lib.load().vaqhip_multi_encode_set_codes, self._train_rows(X), projected, id_base, return_codes)

    def _encode_set(self, fn, X: np.ndarray, projected: bool, id_base: int, return_codes: bool):
        codes = np.empty((X.shape[0], self.M), np.uint16) if return_codes else None
        _lib.check_multi(fn(self._h, _ptr(X), X.shape[0], 1 if projected else 0, int(id_base),
                            _ptr(codes) if return_codes else None))
        return codes

    def _encode_add(self, fn, X: np.ndarray, projected: bool, return_codes: bool):
        codes = np.empty((X.shape[0], self.M), np.uint16) if return_codes else None
        _lib.check_multi(fn(self._h, _ptr(X), X.shape[0], 1 if projected else 0, _ptr(codes) if return_codes else None))
        return codes

    def encode_u8(self, X, projected: bool = True, id_base: int = 0, return_codes: bool = False):
        """encode() from byte rows (vaqhip_multi_encode_set_codes_u8): every shard uploads its slice as bytes; the
        state encode() leaves from X.astype(float32).  Anything but a contiguous uint8 n x D array is EINVAL."""
        return self._encode_set(_lib.load().vaqhip_multi_encode_set_codes_u8, _u8_rows(X, self.D), projected, id_base, return_codes)

    def encode_add_u8(self, X, projected: bool = True, return_codes: bool = False):
        """encode_add() from byte rows (vaqhip_multi_encode_add_codes_u8)."""
        return self._encode_add(_lib.load().vaqhip_multi_encode_add_codes_u8, _u8_rows(X, self.D), projected, return_codes)

    def encode_lut_u8(self, X, projected: bool = True, id_base: int = 0, return_codes: bool = False):
        """encode_lut() from byte rows (vaqhip_multi_encode_lut_set_codes_u8)."""
        return self._encode_set(_lib.load().vaqhip_multi_encode_lut_set_codes_u8, _u8_rows(X, self.D), projected, id_base, return_codes)

    def encode_lut_add_u8(self, X, projected: bool = True, return_codes: bool = False):
        """encode_lut_add() from byte rows (vaqhip_multi_encode_lut_add_codes_u8)."""
        return self._encode_add(_lib.load().vaqhip_multi_encode_lut_add_codes_u8, _u8_rows(X, self.D), projected, return_codes)

    def encode_add(self, X, projected: bool = True, return_codes: bool = False):
        """vaqhip_multi_encode_add_codes: encode + add_codes; the rows extend the last shard and are encoded on its
        device.  ESTATE on an index that never received codes."""
        return self._encode_add(_lib.load().vaqhip_multi_encode_add_codes, self._train_rows(X), projected, return_codes)

    def encode_from_refiner(self, refiner: "VaqMultiRefiner", return_codes: bool = False):
        """vaqhip_multi_encode_from_refiner: encode the RAW rows resident in a multi refiner on the same devices where
        they lie (projected = False); N, id_base and the cut are the refiner's, so search_refine fits afterwards."""
        return self._encode_refiner(_lib.load().vaqhip_multi_encode_from_refiner, refiner, return_codes)

    def _encode_refiner(self, fn, refiner, return_codes: bool):
        codes = np.empty((refiner.info()["N"], self.M), np.uint16) if return_codes else None
        _lib.check_multi(fn(self._h, refiner._h, _ptr(codes) if return_codes else None))
        return codes

    def set_lut_quantiles(self, q) -> None:
        """vaqhip_multi_set_lut_quantiles: Q (D x 257, as the fit writes it) on every shard of a sequential_sum index;
        the encode_lut calls need it."""
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.shape != (self.M, 257):
            raise _lib.VaqHipError(-1, f"quantiles {qq.shape} are not {self.M} x 257")
        _lib.check_multi(_lib.load().vaqhip_multi_set_lut_quantiles(self._h, _ptr(qq)))

    def encode_lut(self, X, projected: bool = True, id_base: int = 0, return_codes: bool = False):
        """encode() with the engine's rule (encodeToLUTCode, VaqHip.encodeLUT) in the place of VAQ::encode's: the state
        VaqHip.encodeLUT on one index followed by set_codes(codes, id_base) leaves, bit for bit."""
        return self._encode_set(_lib.load().vaqhip_multi_encode_lut_set_codes, self._train_rows(X), projected, id_base, return_codes)

    def encode_lut_add(self, X, projected: bool = True, return_codes: bool = False):
        """encode_add() with the engine's rule: the rows extend the last shard and are encoded on its device."""
        return self._encode_add(_lib.load().vaqhip_multi_encode_lut_add_codes, self._train_rows(X), projected, return_codes)

    def encode_lut_from_refiner(self, refiner: "VaqMultiRefiner", return_codes: bool = False):
        """encode_from_refiner() with the engine's rule over the RAW rows resident in a multi refiner."""
        return self._encode_refiner(_lib.load().vaqhip_multi_encode_lut_from_refiner, refiner, return_codes)

    def last_encode_timing(self) -> dict:
        t = _lib.MultiEncodeTiming()
        _lib.check_multi(_lib.load().vaqhip_multi_last_encode_timing(self._h, C.byref(t)))
        return _struct_dict(t)

    def set_option(self, key: str, value: int) -> None:
        """vaqhip_multi_set_option: "exchange" (0 auto, 1 RCCL, 2 copies), "exact_batch" and "encode_chunk_rows" (rows
        per upload chunk of encode(), 0 = 1 << 20) belong to the
        multi index, everything else is forwarded to every shard.  "exact_ties" = 1 holds across the
        shards: labels and distances equal VAQ::search's over ALL rows slot for slot -- every shard scans
        with k + 1, the merged list decides which queries have ties, and those are replayed through the
        reference's heap as a chain from shard to shard (k * 8 bytes per tied query per shard boundary;
        "exact_batch" = list entries per batch of that chain, 0 = automatic).  On sequential-sum shards
        the answer is BitVecEngine::queryLUT's: the chain hands on its std heap of k + 1 pairs, the heap's
        length and bsfK, (k + 2) * 8 bytes per tied query per shard boundary.  No effect at
        k = 1024, and none with TI on several shards (on ONE index the option replays the reference's walk;
        a cluster's member order is one std::sort over rows of all shards and does not decompose into a
        chain)."""
        _lib.check_multi(_lib.load().vaqhip_multi_set_option(self._h, key.encode(), int(value)))

    def set_method(self, methods: int, visit: float = 1.0) -> None:
        _lib.check_multi(_lib.load().vaqhip_multi_set_method(self._h, methods, float(visit)))

    def set_lut_quantization(self, offsets, scale) -> None:
        """vaqhip_multi_set_lut_quantization: mOffsets / mScale of method FAST, the same on every shard.  Call it
        (or learn_quantization) BEFORE set_method(NNMethod.Fast): without a quantisation the multi index refuses
        the method (EUNSUPPORTED)."""
        off = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1)
        sc = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        if off.shape[0] != self.M or sc.shape[0] != self.M:
            raise _lib.VaqHipError(-1, f"offsets {off.shape} / scale {sc.shape}: need {self.M} values each")
        _lib.check_multi(_lib.load().vaqhip_multi_set_lut_quantization(self._h, _ptr(off), _ptr(sc)))

    def learn_quantization(self, XTrain: np.ndarray, sampleRatio: float, projected: bool = False):
        """vaqhip_multi_learn_quantization: VAQ::learnQuantization once, on the first shard, replicated to the
        others.  Returns (offsets, scale), bit-equal to VaqHipFast.learnQuantization on the same rows."""
        X = _f32_rows(XTrain, self.D, "XTrain {shape} is not n x {D}")
        return self._learn_with(lambda off, sc: _lib.load().vaqhip_multi_learn_quantization(
            self._h, _ptr(X), X.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

    def _learn_with(self, call):
        """The arrays around one of the three forms: call(off, sc) -> code; returns (offsets, scale)."""
        off = np.empty(self.M, np.float32)
        sc = np.empty(self.M, np.float32)
        _lib.check_multi(call(_ptr(off), _ptr(sc)))
        return off, sc

    def learn_quantization_u8(self, XTrain: np.ndarray, sampleRatio: float, projected: bool = False):
        """learn_quantization() from byte rows (vaqhip_multi_learn_quantization_u8); anything but a contiguous uint8
        n x D array is EINVAL.  Returns (offsets, scale)."""
        X = _u8_rows(XTrain, self.D)
        return self._learn_with(lambda off, sc: _lib.load().vaqhip_multi_learn_quantization_u8(
            self._h, _ptr(X), X.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

    def learn_quantization_from_refiner(self, refiner: "VaqMultiRefiner", sampleRatio: float):
        """learn_quantization() over the raw rows a VaqMultiRefiner on the same devices holds, read where they are
        (vaqhip_multi_learn_quantization_from_refiner).  Returns (offsets, scale)."""
        return self._learn_with(lambda off, sc: _lib.load().vaqhip_multi_learn_quantization_from_refiner(
            self._h, refiner._h, C.c_float(sampleRatio), off, sc))

    def set_ti_clusters(self, clusters: Optional[np.ndarray], seg: int = 0) -> None:
        if clusters is None:
            _lib.check_multi(_lib.load().vaqhip_multi_set_ti_clusters(self._h, None, 0, 0))
            return
        cl = np.ascontiguousarray(clusters, dtype=np.float32)
        _lib.check_multi(_lib.load().vaqhip_multi_set_ti_clusters(self._h, _ptr(cl), cl.shape[0], seg))

    def cluster_ti_kmeans(self, T: int, seg: int, max_iter: int = 50):
        """vaqhip_multi_cluster_ti_kmeans: the k-means of VAQ::clusterTI(true) over all rows of the shards -- the
        centres a single VaqHip computes over the same rows, bit for bit, whatever the number of shards -- then
        set_ti_clusters with them.  Returns (centres [T, seg * L], iterations, nan_rows)."""
        out = np.empty((max(T, 0), max(seg, 0) * (self.D // self.M)), np.float32)
        iters, nan_rows = C.c_int(0), C.c_int(0)
        _lib.check_multi(_lib.load().vaqhip_multi_cluster_ti_kmeans(self._h, T, seg, max_iter, _ptr(out),
                                                                    C.byref(iters), C.byref(nan_rows)))
        return out, iters.value, nan_rows.value

    def last_kmeans_timing(self) -> dict:
        t = _lib.KmeansTiming()
        _lib.check_multi(_lib.load().vaqhip_multi_last_kmeans_timing(self._h, C.byref(t)))
        return _struct_dict(t)

    def search(self, XTest: np.ndarray, k: int, projected: bool = False) -> LabelDistVec:
        X = np.ascontiguousarray(XTest, dtype=np.float32)
        nq = X.shape[0]
        ret = _new_answer(nq * k)
        _lib.check_multi(_lib.load().vaqhip_multi_search(self._h, _ptr(X), nq, k, 1 if projected else 0,
                                                         _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def search_device(self, d_queries, k: int, projected: bool = False, out=None):
        """vaqhip_multi_search_device: torch CUDA tensors on the FIRST device of the list in and out,
        enqueued behind torch's current stream of that device; nothing is synchronised."""
        q, nq = self._queries_device(d_queries)
        labels, dists = _out_pair(out, nq, k, q.device)
        _lib.check_multi(_lib.load().vaqhip_multi_search_device(
            self._h, _dptr(q), nq, k, 1 if projected else 0, _dptr(labels), _dptr(dists), _stream(q)))
        return labels, dists

    def _queries_device(self, d_queries):
        import torch
        q = d_queries.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.shape[1] == self.D
        return q, q.shape[0]

    def search_refine(self, XTest: np.ndarray, R: int, k: int, refiner: "VaqMultiRefiner") -> LabelDistVec:
        """search(XTest, R) followed by VAQ::refine to k against the multi refiner's sharded rows, in one call
        (vaqhip_multi_search_refine): the candidates go from the merge on the first device straight into the refine.
        Equals search() + refiner.refine() on the same inputs; this index's options apply to the search half."""
        X = _f32_rows(XTest, self.D, "XTest {shape} is not nq x {D}")
        nq = X.shape[0]
        ret = _new_answer(nq * k)
        _lib.check_multi(_lib.load().vaqhip_multi_search_refine(self._h, refiner._h, _ptr(X), nq, int(R), int(k),
                                                                _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def search_refine_device(self, d_queries, R: int, k: int, refiner: "VaqMultiRefiner", out=None):
        """vaqhip_multi_search_refine_device: torch CUDA tensors on the first device, enqueue only."""
        q, nq = self._queries_device(d_queries)
        labels, dists = _out_pair(out, nq, k, q.device)
        _lib.check_multi(_lib.load().vaqhip_multi_search_refine_device(
            self._h, refiner._h, _dptr(q), nq, int(R), int(k), _dptr(labels), _dptr(dists), _stream(q)))
        return labels, dists

    def shard(self, g: int):
        """vaqhip_multi_shard: the raw handle of shard g's single-device index (owned by the multi index)."""
        return _lib.load().vaqhip_multi_shard(self._h, g)

    def info(self) -> dict:
        inf = _lib.MultiInfo()
        _lib.check_multi(_lib.load().vaqhip_multi_get_info(self._h, C.byref(inf)))
        return _struct_dict(inf, cut=("device_ids", "shard_rows"))

