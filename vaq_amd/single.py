"""Python mirror of the reference's `class VAQ` search interface
(bitvecengine/VAQ.hpp:36-113) over the C ABI of include/vaqhip.h.

Member names follow the reference (mBitsAlloc, mCentroidsPerSubs, mCodebook,
mEigenVectors, mMethods ...) so harness code reads like the reference's
drivers (examples/demo_vaq.cpp:58-345).  All compute goes through
libvaqhip.so; nothing here has a NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._adapt import (_Handle, _dptr, _eig_f32, _f32_rows, _out_pair, _ptr, _same, _stream, _struct_dict, _torch_stream,
                     _u8_rows, _u8_rows_device, _wref)
from .fits import lut_fit_quantiles_multi, lut_fit_quantiles_multi_u8


class NNMethod:
    """VAQ::NNMethod bit flags (VAQ.hpp:38-49)."""
    Sort = 0x01
    EA = 0x02
    TI = 0x04
    Fast = 0x08
    Fast2 = 0x10
    Fast3 = 0x20
    Fast4 = 0x40
    Heap = 0x80


@dataclass
class LabelDistVec:
    """utils/Types.hpp:98-104: flat nq*k labels / distances."""
    labels: np.ndarray = field(default_factory=lambda: np.empty(0, np.int32))
    distances: np.ndarray = field(default_factory=lambda: np.empty(0, np.float32))


def _new_answer(n: int) -> LabelDistVec:
    """n slots for a call to fill."""
    return LabelDistVec(np.empty(n, np.int32), np.empty(n, np.float32))


class VaqHip(_Handle):
    """Drop-in for the search half of `class VAQ`.

    Typical use (mirrors demo_vaq.cpp:58-345)::

        vaq = VaqHip()
        vaq.parseMethodString("VAQ64m8min8max8var1,HEAP")
        vaq.mBitsAlloc = [8] * 8
        vaq.mCentroidsPerSubs = [...]          # K_s x L float32 each
        vaq.mEigenVectors = E                  # D x D (real part), or None
        vaq.mCodebook = codes                  # N x M uint16 (CodebookType)
        ans = vaq.search(XTest, 100)           # LabelDistVec

    The FAST method (uint8 tables over codes of at most 4 bits) lives in the
    subclass VaqHipFast: it needs members this class does not have (mOffsets,
    mScale, learnQuantization), and VaqHip keeps refusing FAST in
    parseMethodString so that a drop-in caller asking for it without them
    gets an error instead of a search with no quantisation.
    """

    _destroy = "vaqhip_index_destroy"
    # NNMethod bits parseMethodString accepts and search runs
    _METHODS = NNMethod.Heap | NNMethod.EA | NNMethod.TI

    def __init__(self, device: int = 0, sequential_sum: bool = False):
        """sequential_sum=True: BitVecEngine::queryLUT's arithmetic (one scalar
        quantiser per dimension, columns summed one by one; M need not be a
        multiple of 4) instead of VAQ::searchHeap's groups of four."""
        self.device = device
        self.sequential_sum = sequential_sum
        # VAQ.hpp:51-55
        self.mBitBudget = 0
        self.mSubspaceNum = 0
        self.mPercentVarExplained = 1.0
        self.mMinBitsPerSubs = 0
        self.mMaxBitsPerSubs = 0
        self.mMethods = NNMethod.Heap
        # VAQ.hpp:57-75
        self.mEigenVectors: Optional[np.ndarray] = None
        self.mCentroidsPerSubs: List[np.ndarray] = []
        self.mBitsAlloc: List[int] = []
        self.mCodebook: Optional[np.ndarray] = None
        # VAQ.hpp:77-84: triangle-inequality clusters
        self.mTIClusterNum = 0
        self.mTISegmentNum = -1
        self.mTIVariance = 1.0
        self.mVisit = 1.0
        self.mTIClusters: Optional[np.ndarray] = None  # T x (mTISegmentNum * mSubsLen)
        self.id_base = 0
        self._h = C.c_void_p()
        self._sig = None
        self._codes_sig = None
        self._ti_sig = None
        self._method_sig = None

    # ------------------------------------------------------------ parsing --
    def parseMethodString(self, methodString: str) -> None:
        """VAQ::parseMethodString (VAQ.cpp:1189-1267).  HEAP, EA and TI<T>[m<seg>]
        select the scans on this path; the other tokens the reference accepts
        (SORT, FAST*) are outside it and raise (FAST: see VaqHipFast)."""
        for token in methodString.split(","):
            if token.startswith("VAQ"):
                m = re.match(r"VAQ(\d+)m(\d+)min(\d+)max(\d+)var([0-9.]+)", token)
                if m:
                    self.mBitBudget = int(m.group(1))
                    self.mSubspaceNum = int(m.group(2))
                    self.mMinBitsPerSubs = int(m.group(3))
                    self.mMaxBitsPerSubs = int(m.group(4))
                    self.mPercentVarExplained = float(m.group(5))
            elif any(t in token for t in ("SORT", "HEAP", "EA", "TI", "FAST")):
                methods = 0
                for t in token.split("_"):
                    if "SORT" in t:
                        methods |= NNMethod.Sort
                    elif "HEAP" in t:
                        methods |= NNMethod.Heap
                    elif "EA" in t:
                        methods |= NNMethod.EA
                    elif "TI" in t:
                        # VAQ.cpp:1236-1251: TI<T>var<v> | TI<T>m<seg> | TI<T>
                        mv = re.match(r"TI(\d+)var([0-9.]+)", t)
                        mm = re.match(r"TI(\d+)m(\d+)", t)
                        m1 = re.match(r"TI(\d+)", t)
                        if mv:
                            methods |= NNMethod.TI
                            self.mTIClusterNum = int(mv.group(1))
                            self.mTIVariance = float(mv.group(2))
                        elif mm:
                            methods |= NNMethod.TI
                            self.mTIClusterNum = int(mm.group(1))
                            self.mTISegmentNum = int(mm.group(2))
                        elif m1:
                            methods |= NNMethod.TI
                            self.mTIClusterNum = int(m1.group(1))
                    elif "FAST3" in t:
                        methods |= NNMethod.Fast3
                    elif "FAST2" in t:
                        methods |= NNMethod.Fast2
                    elif "FAST" in t:
                        methods |= NNMethod.Fast
                unsupported = methods & ~self._METHODS
                if unsupported:
                    raise _lib.VaqHipError(-2, f"search method bits 0x{unsupported:02x} in "
                                               f"'{token}' are outside the HEAP/EA/TI path")
                self.mMethods = methods

    def searchMethod(self) -> int:
        return self.mMethods

    # ------------------------------------------------------- derived state --
    @property
    def mHighestSubs(self) -> int:
        return len(self.mBitsAlloc)

    @property
    def mCentroidsNum(self) -> List[int]:
        return [1 << b for b in self.mBitsAlloc]

    @property
    def mTotalDim(self) -> int:
        return sum(c.shape[1] for c in self.mCentroidsPerSubs)

    @property
    def mSubsLen(self) -> int:
        return self.mCentroidsPerSubs[0].shape[1]

    # --------------------------------------------------------------- sync --
    def _ensure_index(self):
        L = _lib.load()
        M = len(self.mBitsAlloc)
        if M == 0 or len(self.mCentroidsPerSubs) != M:
            raise _lib.VaqHipError(-1, "mBitsAlloc / mCentroidsPerSubs not set consistently")
        cents = [np.ascontiguousarray(c, dtype=np.float32) for c in self.mCentroidsPerSubs]
        for b, c in zip(self.mBitsAlloc, cents):
            if c.ndim != 2 or c.shape[0] != (1 << b):
                raise _lib.VaqHipError(-1, f"centroid matrix {c.shape} does not match {b} bits")
        D = sum(c.shape[1] for c in cents)
        eig = _eig_f32(self.mEigenVectors, D, "mEigenVectors")
        plain = (tuple(self.mBitsAlloc), self.device, self.sequential_sum)
        if (self._h and self._sig is not None and self._sig[0] == plain
                and len(self._sig[1]) == M and all(_same(r, c) for r, c in zip(self._sig[1], self.mCentroidsPerSubs))
                and _same(self._sig[2], self.mEigenVectors)):
            return
        sig = (plain, tuple(_wref(c) for c in self.mCentroidsPerSubs), _wref(self.mEigenVectors))
        self.close()
        bits = (C.c_int * M)(*self.mBitsAlloc)
        arr = (C.POINTER(C.c_float) * M)()
        for i, c in enumerate(cents):
            arr[i] = c.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        _lib.check(L.vaqhip_index_create_ex(C.byref(h), D, M, bits, arr,
                                            _ptr(eig) if eig is not None else None, self.device,
                                            1 if self.sequential_sum else 0))
        self._h = h
        self._sig = sig
        self._codes_sig = None
        self._ti_sig = None
        self._method_sig = None

    # ---------------------------------------------------------------- TI --
    def decodeFirstSegments(self, rows: np.ndarray, seg: int) -> np.ndarray:
        """Rows of mCodebook as the vectors clusterTI works on: the centroids of
        their first `seg` codes side by side (VAQ.cpp:926-933)."""
        cb = np.asarray(self.mCodebook)[rows]
        return np.concatenate([np.asarray(self.mCentroidsPerSubs[s], np.float32)[cb[:, s].astype(np.int64)]
                               for s in range(seg)], axis=1)

    def clusterTI(self, useKMeans: bool = False, verbose: bool = False, seed: int = 13517106) -> None:
        """VAQ::clusterTI (VAQ.hpp:106, VAQ.cpp:878-999).  Makes mTIClusters when it
        is not set yet -- useKMeans=False: mTIClusterNum random code rows, decoded
        (VAQ.cpp:901-911, drawn with `seed`); True: the reference's k-means over decoded
        code rows (:897-900, KMeans::staticFitCodebook, 50 iterations at most) on the GPU,
        centre for centre what the reference computes (vaqhip_index_cluster_ti_kmeans;
        kmeansIterations / kmeansNanRows tell how it ended) -- and leaves the grouping
        itself (:913-996) to the GPU: at once with the k-means, else at the next search."""
        if self.mTIVariance < 1:
            raise _lib.VaqHipError(-2, "TI<T>var<v> needs train()'s variance profile; use TI<T>m<seg>")
        seg = self.mTISegmentNum if self.mTISegmentNum != -1 else self.mHighestSubs  # :890-892
        self.mTISegmentNum = seg
        if self.mTIClusters is None and useKMeans:
            # the codes go to the device first, in the exhaustive order (no centres yet)
            methods = self.mMethods
            self.mMethods = (methods & ~NNMethod.TI) or NNMethod.Heap
            try:
                self._ensure_codes()
            finally:
                self.mMethods = methods
            T = self.mTIClusterNum
            out = np.empty((max(T, 0), seg * self.mSubsLen), np.float32)
            iters, nan_rows = C.c_int(0), C.c_int(0)
            _lib.check(_lib.load().vaqhip_index_cluster_ti_kmeans(self._h, T, seg, 50, _ptr(out), C.byref(iters),
                                                                  C.byref(nan_rows)))
            self.mTIClusters = out
            self.kmeansIterations, self.kmeansNanRows = iters.value, nan_rows.value
            self._ti_sig = (_wref(out), seg)  # the index holds these centres already
        elif self.mTIClusters is None:
            if self.mCodebook is None or hasattr(self.mCodebook, "data_ptr"):
                raise _lib.VaqHipError(-7, "clusterTI needs a host mCodebook (or set mTIClusters)")
            T = self.mTIClusterNum
            N = self.mCodebook.shape[0]
            rng = np.random.default_rng(seed)
            self.mTIClusters = self.decodeFirstSegments(rng.integers(0, N, size=T), seg)
        self.mMethods |= NNMethod.TI

    def _ensure_ti(self):
        L = _lib.load()
        if self.mMethods & NNMethod.TI:
            if self.mTIClusters is None:
                raise _lib.VaqHipError(-7, "method TI: call clusterTI() or set mTIClusters first")
            cl = np.ascontiguousarray(self.mTIClusters, dtype=np.float32)
            seg = self.mTISegmentNum if self.mTISegmentNum != -1 else self.mHighestSubs
            if cl.ndim != 2 or cl.shape[1] != seg * self.mSubsLen:
                raise _lib.VaqHipError(-1, f"mTIClusters {cl.shape} is not T x {seg * self.mSubsLen}")
            if self._ti_sig is None or self._ti_sig[1] != seg or not _same(self._ti_sig[0], self.mTIClusters):
                _lib.check(L.vaqhip_index_set_ti_clusters(self._h, _ptr(cl), cl.shape[0], seg))
                self._ti_sig = (_wref(self.mTIClusters), seg)
        elif self._ti_sig is not None:
            _lib.check(L.vaqhip_index_set_ti_clusters(self._h, None, 0, 0))
            self._ti_sig = None
        msig = (self.mMethods, float(self.mVisit))
        if msig != self._method_sig:
            _lib.check(L.vaqhip_index_set_method(self._h, self.mMethods, float(self.mVisit)))
            self._method_sig = msig

    def _ensure_codes(self):
        self._ensure_index()
        self._ensure_ti()  # before the codes: they are then grouped once, not twice
        if self.mCodebook is None:
            if self._codes_sig is not None:
                return  # the packed copy already lives on the device (host copy was dropped)
            raise _lib.VaqHipError(-7, "mCodebook is not set")
        if (self._codes_sig is not None and self._codes_sig[1] == self.id_base
                and _same(self._codes_sig[0], self.mCodebook)):
            return
        sig = (_wref(self.mCodebook), self.id_base)
        cb = self.mCodebook
        if hasattr(cb, "data_ptr"):  # torch tensor already on the device: N x M int16/uint16
            if cb.dim() != 2 or cb.shape[1] != len(self.mBitsAlloc) or cb.element_size() != 2:
                raise _lib.VaqHipError(-1, "device mCodebook must be N x M 16-bit")
            if not cb.is_cuda or cb.device.index != self.device or not cb.is_contiguous():
                raise _lib.VaqHipError(-1, f"device mCodebook must be a contiguous tensor on cuda:{self.device} "
                                           f"(got {cb.device}, contiguous={cb.is_contiguous()})")
            _lib.check(_lib.load().vaqhip_index_set_codes_u16_device(self._h, _dptr(cb), cb.shape[0], self.id_base, _stream(cb)))
            _torch_stream(cb.device).synchronize()
        else:
            cb = np.ascontiguousarray(cb, dtype=np.uint16)
            if cb.ndim != 2 or cb.shape[1] != len(self.mBitsAlloc):
                raise _lib.VaqHipError(-1, f"mCodebook {cb.shape} is not N x {len(self.mBitsAlloc)}")
            _lib.check(_lib.load().vaqhip_index_set_codes_u16(self._h, _ptr(cb), cb.shape[0],
                                                              self.id_base))
        self._codes_sig = sig

    def add_codes(self, codes: np.ndarray) -> None:
        """Append rows to the index on the device (vaqhip_index_add_codes_u16); the host
        mCodebook, if still attached, grows with them so the two stay the same matrix."""
        self._ensure_codes()
        cb = np.ascontiguousarray(codes, dtype=np.uint16)
        if cb.ndim != 2 or cb.shape[1] != len(self.mBitsAlloc):
            raise _lib.VaqHipError(-1, f"codes {cb.shape} is not n x {len(self.mBitsAlloc)}")
        _lib.check(_lib.load().vaqhip_index_add_codes_u16(self._h, _ptr(cb), cb.shape[0]))
        if self.mCodebook is not None and not hasattr(self.mCodebook, "data_ptr"):
            self.mCodebook = np.concatenate([np.asarray(self.mCodebook, dtype=np.uint16), cb])
            self._codes_sig = (_wref(self.mCodebook), self.id_base)

    # ------------------------------------------------------------- search --
    def search(self, XTest: np.ndarray, k: int, verbose: bool = False,
               projected: bool = False) -> LabelDistVec:
        """VAQ::search (VAQ.cpp:776-847): flat labels / distances, ascending per
        query; squared for HEAP / EA, square roots with TI (VAQ.cpp:1583)."""
        X = self._host_queries(XTest)
        nq = X.shape[0]
        ret = _new_answer(nq * k)
        fn = _lib.load().vaqhip_search_projected if projected else _lib.load().vaqhip_search
        _lib.check(fn(self._h, _ptr(X), nq, k, _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def _host_queries(self, XTest) -> np.ndarray:
        """The start of a host search: the method is one of this path's, the codes are on the device, XTest fits."""
        if not (self.mMethods & self._METHODS):
            raise _lib.VaqHipError(-2, "only HEAP / EA / TI are implemented on this path")
        self._ensure_codes()
        return _f32_rows(XTest, self.mTotalDim, "XTest {shape} is not nq x {D}")

    def search_device(self, d_queries, k: int, projected: bool = False, out=None):
        """Device-resident variant: torch CUDA tensors in and out, enqueued on
        torch's current stream (no host copies, no synchronisation).  out =
        (labels int32 [nq,k], distances float32 [nq,k]) reuses caller buffers, so a
        steady-state loop performs no allocation at all."""
        import torch
        self._ensure_codes()
        q = d_queries.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.shape[1] == self.mTotalDim
        nq = q.shape[0]
        labels, dists = _out_pair(out, nq, k, q.device)
        if out is not None:
            assert labels.shape == (nq, k) and labels.dtype == torch.int32 and labels.is_contiguous()
            assert dists.shape == (nq, k) and dists.dtype == torch.float32 and dists.is_contiguous()
        _lib.check(_lib.load().vaqhip_search_device(
            self._h, _dptr(q), nq, k, 1 if projected else 0, _dptr(labels), _dptr(dists), _stream(q)))
        return labels, dists

    # ----------------------------------------------- staged search (sharded hosts) --
    def staged_supported(self, nq: int, k: int) -> bool:
        """vaqhip_search_staged_supported: would a search of nq queries run the bucket-major rounds,
        i.e. can it be split around a threshold exchange between shards?"""
        self._ensure_codes()
        return bool(_lib.load().vaqhip_search_staged_supported(self._h, int(nq), int(k)))

    def search_begin_device(self, d_queries, k: int, out, thr_out, projected: bool = False) -> None:
        """vaqhip_search_begin_device: first rounds; thr_out (int32 [nq], CUDA) receives the thresholds
        (distance bits) to be MIN-reduced over the shards; out = (labels, dists) as for search_device."""
        import torch
        self._ensure_codes()
        q = d_queries.contiguous()
        labels, dists = out
        nq = q.shape[0]
        assert thr_out.is_cuda and thr_out.dtype == torch.int32 and thr_out.numel() == nq and thr_out.is_contiguous()
        _lib.check(_lib.load().vaqhip_search_begin_device(
            self._h, _dptr(q), nq, k, 1 if projected else 0, _dptr(labels), _dptr(dists), _dptr(thr_out), _stream(q)))

    def search_finish_device(self, thr_in=None) -> None:
        """vaqhip_search_finish_device: the rest of the search under the exchanged thresholds."""
        import torch
        dev = thr_in.device if thr_in is not None else torch.device("cuda", self.device)
        _lib.check(_lib.load().vaqhip_search_finish_device(
            self._h, _dptr(thr_in) if thr_in is not None else None, C.c_void_p(_torch_stream(dev).cuda_stream)))

    # ----------------------------------------------------- encode / refine --
    def encode(self, XTrain: np.ndarray, projected: bool = True) -> None:
        """VAQ::encode (VAQ.cpp:663-748): fills mCodebook (N x M uint16).  Like
        the reference it expects rows already in PCA space (train() projects the
        dataset in place); projected=False applies mEigenVectors first."""
        self._ensure_index()
        X = np.ascontiguousarray(XTrain, dtype=np.float32)
        self._encode_host(_lib.load().vaqhip_encode, X, projected)

    def _encode_host(self, fn, X: np.ndarray, projected: bool) -> None:
        codes = np.empty((X.shape[0], len(self.mBitsAlloc)), np.uint16)
        _lib.check(fn(self._h, _ptr(X), X.shape[0], 1 if projected else 0, _ptr(codes)))
        self.mCodebook = codes

    def encode_u8(self, XTrain: np.ndarray, projected: bool = True) -> None:
        """encode() from byte rows (a bvecs dataset as its file holds it; vaqhip_encode_u8): the codes encode() gives
        on XTrain.astype(float32), code for code, from a quarter of the upload.  Anything but a contiguous uint8
        n x D array is EINVAL: nothing is converted."""
        X = _u8_rows(XTrain, self.mTotalDim)
        self._ensure_index()
        self._encode_host(_lib.load().vaqhip_encode_u8, X, projected)

    def encode_device(self, d_X, projected: bool = True):
        """torch CUDA tensor in, N x M int16 CUDA tensor (uint16 codes) out, on
        torch's current stream."""
        import torch
        self._ensure_index()
        x = d_X.contiguous()
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[1] == self.mTotalDim
        return self._encode_on_device(_lib.load().vaqhip_encode_device, x, projected)

    def _encode_on_device(self, fn, x, projected: bool):
        import torch
        codes = torch.empty((x.shape[0], len(self.mBitsAlloc)), dtype=torch.int16, device=x.device)
        _lib.check(fn(self._h, _dptr(x), x.shape[0], 1 if projected else 0, _dptr(codes), _stream(x)))
        return codes

    def encode_u8_device(self, d_X, projected: bool = True):
        """encode_device() from a torch uint8 CUDA tensor (vaqhip_encode_u8_device); it may start at any byte."""
        x = _u8_rows_device(d_X, self.mTotalDim)
        self._ensure_index()
        return self._encode_on_device(_lib.load().vaqhip_encode_u8_device, x, projected)

    # ------------------------------------------- building a queryLUT index --
    def _need_sequential(self, what: str) -> None:
        if not self.sequential_sum:
            raise _lib.VaqHipError(-1, f"{what} builds BitVecEngine::queryLUT's index: VaqHip(sequential_sum=True)")

    def fitQuantiles(self, XTrain: np.ndarray, projected: bool = True, devices: Optional[Sequence[int]] = None) -> None:
        """BitVecEngine::binaryEncodingLUT's codebooks (BitVecEngine.hpp:811-867) on the GPU: with mBitsAlloc
        (solutionX, 1..8 per dimension) and, for projected=False, mEigenVectors set by the caller -- the PCA
        and the bit allocation stay the caller's --, fills mCentroidsPerSubs (column d of centroidsMat),
        centroidsMat (256 x D) and mQuantiles (D x 257), bit for bit what centroidsQuantile computes
        (vaqhip_lut_fit_quantiles).  A NaN or infinite training value is refused (EINVAL).  devices=[...]: the same
        members from the sharded fit over those devices (lut_fit_quantiles_multi): the rows are cut over them and no
        device holds them all."""
        self._need_sequential("fitQuantiles")
        X = np.ascontiguousarray(XTrain, dtype=np.float32)
        D = len(self.mBitsAlloc)
        if X.ndim != 2 or X.shape[1] != D or D == 0:
            raise _lib.VaqHipError(-1, f"XTrain {X.shape} is not n x {D} (one quantiser per dimension)")
        self._fit_quantiles(X, projected, devices, False)

    def fitQuantiles_u8(self, XTrain: np.ndarray, projected: bool = True, devices: Optional[Sequence[int]] = None) -> None:
        """fitQuantiles() from byte rows (vaqhip_lut_fit_quantiles_u8, or lut_fit_quantiles_multi_u8 with devices):
        the members fitQuantiles() fills from XTrain.astype(float32), bit for bit.  Anything but a contiguous uint8
        n x D array is EINVAL."""
        self._need_sequential("fitQuantiles_u8")
        self._fit_quantiles(_u8_rows(XTrain, len(self.mBitsAlloc)), projected, devices, True)

    def _fit_quantiles(self, X: np.ndarray, projected: bool, devices, u8: bool) -> None:
        D = len(self.mBitsAlloc)
        L = _lib.load()
        eig = None if projected else _eig_f32(self.mEigenVectors, D, "mEigenVectors")
        if devices is not None:
            cent, q = (lut_fit_quantiles_multi_u8 if u8 else lut_fit_quantiles_multi)(devices, X, self.mBitsAlloc, eig)
        else:
            cent = np.empty((D, 256), np.float32)
            q = np.empty((D, 257), np.float32)
            fit = L.vaqhip_lut_fit_quantiles_u8 if u8 else L.vaqhip_lut_fit_quantiles
            _lib.check(fit(self.device, _ptr(X), X.shape[0], D, (C.c_int * max(D, 1))(*self.mBitsAlloc),
                           _ptr(eig) if eig is not None else None, _ptr(cent), _ptr(q)))
        self.centroidsMat = np.ascontiguousarray(cent.T)
        self.mCentroidsPerSubs = [np.ascontiguousarray(cent[d, :1 << b].reshape(-1, 1)) for d, b in enumerate(self.mBitsAlloc)]
        self.mQuantiles = q

    def _ensure_quantiles(self) -> None:
        self._need_sequential("encodeLUT")
        q = getattr(self, "mQuantiles", None)
        if q is None:
            raise _lib.VaqHipError(-7, "encodeLUT needs mQuantiles: call fitQuantiles first")
        self._ensure_index()
        sig = getattr(self, "_lutq_sig", None)
        if sig is not None and sig[0] == self._h.value and _same(sig[1], q):
            return
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.shape != (len(self.mBitsAlloc), 257):
            raise _lib.VaqHipError(-1, f"mQuantiles {qq.shape} is not {len(self.mBitsAlloc)} x 257")
        _lib.check(_lib.load().vaqhip_index_set_lut_quantiles(self._h, _ptr(qq)))
        self._lutq_sig = (self._h.value, _wref(q))

    def encodeLUT(self, XTrain: np.ndarray, projected: bool = True) -> None:
        """encodeToLUTCode (BitVecEngine.hpp:889-932): fills mCodebook (N x D uint16) with the engine's own
        choice among the centres around a row's quantile bucket -- not encode()'s first argmin."""
        self._ensure_quantiles()
        X = _f32_rows(XTrain, len(self.mBitsAlloc), "XTrain {shape} is not n x {D}")
        self._encode_host(_lib.load().vaqhip_encode_lut, X, projected)

    def encodeLUT_u8(self, XTrain: np.ndarray, projected: bool = True) -> None:
        """encodeLUT() from byte rows (vaqhip_encode_lut_u8): the codes of encodeLUT() on XTrain.astype(float32)."""
        X = _u8_rows(XTrain, len(self.mBitsAlloc))
        self._ensure_quantiles()
        self._encode_host(_lib.load().vaqhip_encode_lut_u8, X, projected)

    def encodeLUT_device(self, d_X, projected: bool = True):
        """torch CUDA tensor in, N x D int16 CUDA tensor (uint16 codes) out, on torch's current stream: the layout
        mCodebook takes as a device tensor, so a build never leaves the device."""
        import torch
        self._ensure_quantiles()
        x = d_X.contiguous()
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[1] == len(self.mBitsAlloc)
        return self._encode_on_device(_lib.load().vaqhip_encode_lut_device, x, projected)

    def encodeLUT_u8_device(self, d_X, projected: bool = True):
        """encodeLUT_device() from a torch uint8 CUDA tensor (vaqhip_encode_lut_u8_device); it may start at any byte."""
        x = _u8_rows_device(d_X, len(self.mBitsAlloc))
        self._ensure_quantiles()
        return self._encode_on_device(_lib.load().vaqhip_encode_lut_u8_device, x, projected)

    def refine(self, XTest: np.ndarray, answersIn: LabelDistVec, XTrain: np.ndarray, k: int) -> LabelDistVec:
        """VAQ::refine (VAQ.cpp:849-876): exact re-rank of the candidates in
        answersIn against the raw dataset XTrain."""
        _lib.load()
        Xq = np.ascontiguousarray(XTest, dtype=np.float32)
        Xt = np.ascontiguousarray(XTrain, dtype=np.float32)
        nq = Xq.shape[0]
        lab = np.ascontiguousarray(answersIn.labels, dtype=np.int32)
        R = lab.size // max(nq, 1)
        ret = _new_answer(nq * k)
        _lib.check(_lib.load().vaqhip_refine(self.device, _ptr(Xq), nq, Xq.shape[1], _ptr(Xt), Xt.shape[0],
                                             _ptr(lab), R, k, _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def search_refine(self, XTest: np.ndarray, R: int, k: int, refiner: "VaqRefiner") -> LabelDistVec:
        """search(XTest, R) followed by VAQ::refine to k against the refiner's resident rows, in one call
        (vaqhip_search_refine): the R candidates per query never leave the device.  The search runs under this
        index's own method and options; the result equals search() + refiner.refine() on the same inputs."""
        X = self._host_queries(XTest)
        nq = X.shape[0]
        ret = _new_answer(nq * k)
        _lib.check(_lib.load().vaqhip_search_refine(self._h, refiner._h, _ptr(X), nq, int(R), int(k), _ptr(ret.labels),
                                                    _ptr(ret.distances)))
        return ret

    # -------------------------------------------------------- test hooks ---
    def build_lut(self, XTest: np.ndarray, projected: bool = False) -> np.ndarray:
        """CreateLUT for every query in the reference's LUTType layout:
        returns (nq, M, ksub) with lut[q, s, c] (column-major ksub x M per query)."""
        self._ensure_index()
        X = np.ascontiguousarray(XTest, dtype=np.float32)
        nq = X.shape[0]
        ksub = 1 << max(self.mBitsAlloc)
        out = np.empty((nq, len(self.mBitsAlloc), ksub), np.float32)
        _lib.check(_lib.load().vaqhip_build_lut(self._h, _ptr(X), nq, 1 if projected else 0,
                                                _ptr(out)))
        return out

    def project(self, X: np.ndarray) -> np.ndarray:
        """VAQ::ProjectOnEigenVectors (VAQ.hpp:198-201)."""
        self._ensure_index()
        X = np.ascontiguousarray(X, dtype=np.float32)
        out = np.empty_like(X)
        _lib.check(_lib.load().vaqhip_project(self._h, _ptr(X), X.shape[0], _ptr(out)))
        return out

    def invalidate(self) -> None:
        """Members are re-uploaded when they are REPLACED (a different object); after editing
        mCodebook, the centroid matrices, mEigenVectors or mTIClusters IN PLACE call this so
        that the next search rebuilds the device index from the current contents."""
        self.close()
        self._ti_sig = None
        self._method_sig = None

    def set_option(self, key: str, value: int) -> None:
        """vaqhip_set_option (include/vaqhip.h lists the options).  "exact_ties" = 1: labels and distances
        identical to VAQ::search's slot for slot -- HEAP / EA through the reference's heap (k < 1024), and on
        a TI index (mTIClusters set, methods TI and TI | EA, any mVisit, k <= 1024) every query is a replay
        of VAQ::searchTriangleInequality over the cluster order and the member order libstdc++'s std::sort
        leaves, NaN centres included."""
        self._ensure_index()
        _lib.check(_lib.load().vaqhip_set_option(self._h, key.encode(), int(value)))

    def info(self) -> dict:
        self._ensure_index()
        inf = _lib.Info()
        _lib.check(_lib.load().vaqhip_index_info(self._h, C.byref(inf)))
        return _struct_dict(inf)

    def last_timing(self) -> dict:
        t = _lib.Timing()
        _lib.check(_lib.load().vaqhip_last_timing(self._h, C.byref(t)))
        return _struct_dict(t)

    def last_learn_timing(self) -> dict:
        """Figures of the last device-form learnQuantization on this index (vaqhip_last_learn_timing): the sample,
        the column groups, the chosen alpha, the phases' host-clock times and the seven alphas' losses."""
        t = _lib.LearnTiming()
        _lib.check(_lib.load().vaqhip_last_learn_timing(self._h, C.byref(t)))
        d = _struct_dict(t)
        d["loss"] = np.array(d["loss"], np.float64)
        return d

    def last_kmeans_timing(self) -> dict:
        """Figures of the last clusterTI(True) on this index (vaqhip_last_kmeans_timing)."""
        t = _lib.KmeansTiming()
        _lib.check(_lib.load().vaqhip_last_kmeans_timing(self._h, C.byref(t)))
        return _struct_dict(t)

    def close(self) -> None:
        if self._h:
            super().close()
            self._sig = None
            self._codes_sig = None

