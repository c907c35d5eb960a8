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
import weakref
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib


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


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


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


class VaqHip:
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
        eig = None
        if self.mEigenVectors is not None:
            eig = np.ascontiguousarray(np.real(self.mEigenVectors), dtype=np.float32)
            if eig.shape != (D, D):
                raise _lib.VaqHipError(-1, f"mEigenVectors {eig.shape} is not {D}x{D}")
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
            import torch
            st = torch.cuda.current_stream(cb.device).cuda_stream
            _lib.check(_lib.load().vaqhip_index_set_codes_u16_device(
                self._h, C.c_void_p(cb.data_ptr()), cb.shape[0], self.id_base, C.c_void_p(st)))
            torch.cuda.current_stream(cb.device).synchronize()
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
        if not (self.mMethods & self._METHODS):
            raise _lib.VaqHipError(-2, "only HEAP / EA / TI are implemented on this path")
        self._ensure_codes()
        X = np.ascontiguousarray(XTest, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.mTotalDim:
            raise _lib.VaqHipError(-1, f"XTest {X.shape} is not nq x {self.mTotalDim}")
        nq = X.shape[0]
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        fn = _lib.load().vaqhip_search_projected if projected else _lib.load().vaqhip_search
        _lib.check(fn(self._h, _ptr(X), nq, k, _ptr(ret.labels), _ptr(ret.distances)))
        return ret

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
        if out is not None:
            labels, dists = out
            assert labels.shape == (nq, k) and labels.dtype == torch.int32 and labels.is_contiguous()
            assert dists.shape == (nq, k) and dists.dtype == torch.float32 and dists.is_contiguous()
        else:
            labels = torch.empty((nq, k), dtype=torch.int32, device=q.device)
            dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        st = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check(_lib.load().vaqhip_search_device(
            self._h, C.c_void_p(q.data_ptr()), nq, k, 1 if projected else 0,
            C.c_void_p(labels.data_ptr()), C.c_void_p(dists.data_ptr()), C.c_void_p(st)))
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
        st = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check(_lib.load().vaqhip_search_begin_device(
            self._h, C.c_void_p(q.data_ptr()), nq, k, 1 if projected else 0, C.c_void_p(labels.data_ptr()),
            C.c_void_p(dists.data_ptr()), C.c_void_p(thr_out.data_ptr()), C.c_void_p(st)))

    def search_finish_device(self, thr_in=None) -> None:
        """vaqhip_search_finish_device: the rest of the search under the exchanged thresholds."""
        import torch
        dev = thr_in.device if thr_in is not None else torch.device("cuda", self.device)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().vaqhip_search_finish_device(
            self._h, C.c_void_p(thr_in.data_ptr()) if thr_in is not None else None, C.c_void_p(st)))

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
        st = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(fn(self._h, C.c_void_p(x.data_ptr()), x.shape[0], 1 if projected else 0,
                      C.c_void_p(codes.data_ptr()), C.c_void_p(st)))
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
        eig = None
        if not projected and self.mEigenVectors is not None:
            eig = np.ascontiguousarray(np.real(self.mEigenVectors), dtype=np.float32)
            if eig.shape != (D, D):
                raise _lib.VaqHipError(-1, f"mEigenVectors {eig.shape} is not {D}x{D}")
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
        X = np.ascontiguousarray(XTrain, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != len(self.mBitsAlloc):
            raise _lib.VaqHipError(-1, f"XTrain {X.shape} is not n x {len(self.mBitsAlloc)}")
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
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        _lib.check(_lib.load().vaqhip_refine(self.device, _ptr(Xq), nq, Xq.shape[1], _ptr(Xt), Xt.shape[0],
                                             _ptr(lab), R, k, _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def search_refine(self, XTest: np.ndarray, R: int, k: int, refiner: "VaqRefiner") -> LabelDistVec:
        """search(XTest, R) followed by VAQ::refine to k against the refiner's resident rows, in one call
        (vaqhip_search_refine): the R candidates per query never leave the device.  The search runs under this
        index's own method and options; the result equals search() + refiner.refine() on the same inputs."""
        if not (self.mMethods & self._METHODS):
            raise _lib.VaqHipError(-2, "only HEAP / EA / TI are implemented on this path")
        self._ensure_codes()
        X = np.ascontiguousarray(XTest, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.mTotalDim:
            raise _lib.VaqHipError(-1, f"XTest {X.shape} is not nq x {self.mTotalDim}")
        nq = X.shape[0]
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
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
        return {f: getattr(inf, f) for f, _ in _lib.Info._fields_}

    def last_timing(self) -> dict:
        t = _lib.Timing()
        _lib.check(_lib.load().vaqhip_last_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in _lib.Timing._fields_}

    def last_learn_timing(self) -> dict:
        """Figures of the last device-form learnQuantization on this index (vaqhip_last_learn_timing): the sample,
        the column groups, the chosen alpha, the phases' host-clock times and the seven alphas' losses."""
        t = _lib.LearnTiming()
        _lib.check(_lib.load().vaqhip_last_learn_timing(self._h, C.byref(t)))
        d = {f: getattr(t, f) for f, _ in _lib.LearnTiming._fields_ if f != "loss"}
        d["loss"] = np.array(list(t.loss), np.float64)
        return d

    def last_kmeans_timing(self) -> dict:
        """Figures of the last clusterTI(True) on this index (vaqhip_last_kmeans_timing)."""
        t = _lib.KmeansTiming()
        _lib.check(_lib.load().vaqhip_last_kmeans_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in _lib.KmeansTiming._fields_}

    def close(self) -> None:
        if self._h:
            _lib.load().vaqhip_index_destroy(self._h)
            self._h = C.c_void_p()
            self._sig = None
            self._codes_sig = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VaqRefiner:
    """The raw rows VAQ::refine reads (VAQ.cpp:849-876), resident on the device, and the reference-exact re-rank
    over them (vaqhip_refiner_*): distances in Eigen's summation order, bit for bit the reference's on any float
    data; with exact_ties also its heap's choice and order among equal distances.

        r = VaqRefiner(D, device=0)
        r.set_rows(XTrain)                       # one upload; row i has label id_base + i
        r.exact_ties = True
        ans = r.refine(XTest, candidates, k)     # candidates: nq x R labels in the order the search returned them
        ans = vaq.search_refine(XTest, R, k, r)  # or fused with the search: the candidates stay on the device
        r.set_rows_u8(io.read_bvecs_u8(path))    # a bvecs dataset kept as bytes: a quarter of the memory, same answers
    """

    def __init__(self, D: int, device: int = 0):
        self.D = int(D)
        self.device = device
        self._exact = False
        self._h = C.c_void_p()
        h = C.c_void_p()
        _lib.check(_lib.load().vaqhip_refiner_create(C.byref(h), device, self.D))
        self._h = h

    def _rows(self, X) -> np.ndarray:
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.D:
            raise _lib.VaqHipError(-1, f"rows {X.shape} are not n x {self.D}")
        return X

    def set_rows(self, XTrain, id_base: int = 0) -> None:
        """Replace the rows: a host array, or a contiguous float32 torch tensor on the refiner's device (copied)."""
        if hasattr(XTrain, "data_ptr"):
            import torch
            x = XTrain
            if not (x.is_cuda and x.device.index == self.device and x.dtype == torch.float32 and x.is_contiguous()
                    and x.dim() == 2 and x.shape[1] == self.D):
                raise _lib.VaqHipError(-1, f"device rows must be a contiguous float32 n x {self.D} tensor on cuda:{self.device}")
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(_lib.load().vaqhip_refiner_set_rows_device(self._h, C.c_void_p(x.data_ptr()), x.shape[0],
                                                                  int(id_base), C.c_void_p(st)))
            return
        X = self._rows(XTrain)
        _lib.check(_lib.load().vaqhip_refiner_set_rows(self._h, _ptr(X), X.shape[0], int(id_base)))

    def add_rows(self, X) -> None:
        """Append rows; their labels continue behind the rows already held."""
        X = self._rows(X)
        _lib.check(_lib.load().vaqhip_refiner_add_rows(self._h, _ptr(X), X.shape[0]))

    def _rows_u8(self, X) -> np.ndarray:
        X = np.asarray(X)
        if X.dtype != np.uint8 or X.ndim != 2 or X.shape[1] != self.D or not X.flags.c_contiguous:
            raise _lib.VaqHipError(-1, f"byte rows must be a contiguous uint8 n x {self.D} array (nothing is converted)")
        return X

    def set_rows_u8(self, XTrain, id_base: int = 0) -> None:
        """Replace the rows by BYTE rows, kept as uint8 on the device (a bvecs dataset as stored): a contiguous np.uint8
        n x D array, or a contiguous torch.uint8 tensor on the refiner's device (copied).  Every call that reads the rows
        answers as over XTrain.astype(float32), bit for bit.  set_rows(uint8 array) still widens to float."""
        if hasattr(XTrain, "data_ptr"):
            import torch
            x = XTrain
            if not (x.is_cuda and x.device.index == self.device and x.dtype == torch.uint8 and x.is_contiguous()
                    and x.dim() == 2 and x.shape[1] == self.D):
                raise _lib.VaqHipError(-1, f"device rows must be a contiguous uint8 n x {self.D} tensor on cuda:{self.device}")
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(_lib.load().vaqhip_refiner_set_rows_u8_device(self._h, C.c_void_p(x.data_ptr()), x.shape[0],
                                                                     int(id_base), C.c_void_p(st)))
            return
        X = self._rows_u8(XTrain)
        _lib.check(_lib.load().vaqhip_refiner_set_rows_u8(self._h, _ptr(X), X.shape[0], int(id_base)))

    def add_rows_u8(self, X) -> None:
        """Append byte rows to byte rows (or to none); ESTATE (-7) on float rows, as add_rows on byte rows."""
        X = self._rows_u8(X)
        _lib.check(_lib.load().vaqhip_refiner_add_rows_u8(self._h, _ptr(X), X.shape[0]))

    @property
    def elem_size(self) -> int:
        """Bytes per element of the rows held: 4 (float32) or 1 (uint8)."""
        return _lib.check(_lib.load().vaqhip_refiner_elem_size(self._h))

    def fit_codebooks(self, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25):
        """fit_codebooks() over the rows held, float or byte, read where they are (vaqhip_refiner_fit_codebooks)."""
        return _fit_codebooks_call(self.D, M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: L.vaqhip_refiner_fit_codebooks(
            self._h, int(M), b, e, it, c, i, nn))

    @property
    def exact_ties(self) -> bool:
        return self._exact

    @exact_ties.setter
    def exact_ties(self, on: bool) -> None:
        _lib.check(_lib.load().vaqhip_refiner_set_option(self._h, b"exact_ties", 1 if on else 0))
        self._exact = bool(on)

    def refine(self, XTest, answersIn, k: int) -> LabelDistVec:
        """answersIn: a LabelDistVec (as search() returns it) or an array of nq * R labels.  Labels that are negative
        or name no resident row are skipped."""
        Xq = self._rows(XTest)
        nq = Xq.shape[0]
        lab = np.ascontiguousarray(getattr(answersIn, "labels", answersIn), dtype=np.int32).reshape(-1)
        R = lab.size // max(nq, 1)
        if nq and lab.size != nq * R:
            raise _lib.VaqHipError(-1, f"{lab.size} labels for {nq} queries")
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        if nq == 0:
            return ret
        _lib.check(_lib.load().vaqhip_refiner_refine(self._h, _ptr(Xq), nq, _ptr(lab), R, int(k), _ptr(ret.labels),
                                                     _ptr(ret.distances)))
        return ret

    def refine_device(self, d_queries, d_labels_in, k: int, out=None):
        """torch CUDA tensors in and out (queries nq x D float32, labels nq x R int32), enqueued on torch's current
        stream, no synchronisation."""
        import torch
        q = d_queries.contiguous()
        lin = d_labels_in.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.shape[1] == self.D
        assert lin.is_cuda and lin.dtype == torch.int32 and lin.shape[0] == q.shape[0]
        nq, R = lin.shape
        if out is not None:
            labels, dists = out
        else:
            labels = torch.empty((nq, k), dtype=torch.int32, device=q.device)
            dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        st = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check(_lib.load().vaqhip_refiner_refine_device(
            self._h, C.c_void_p(q.data_ptr()), nq, C.c_void_p(lin.data_ptr()), R, int(k),
            C.c_void_p(labels.data_ptr()), C.c_void_p(dists.data_ptr()), C.c_void_p(st)))
        return labels, dists

    def set_option(self, key: str, value: int) -> None:
        """"exact_ties", "exhaustive_splits" (0 = automatic, 1..64), "timing"."""
        _lib.check(_lib.load().vaqhip_refiner_set_option(self._h, key.encode(), int(value)))
        if key == "exact_ties":
            self._exact = bool(value)

    def search(self, XTest, k: int) -> LabelDistVec:
        """The exhaustive form of refine(): the candidates are ALL resident rows in row order -- the true k nearest rows
        of every query with the reference's own distances (and, with exact_ties, its heap's choice among equal ones)."""
        Xq = self._rows(XTest)
        nq = Xq.shape[0]
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        _lib.check(_lib.load().vaqhip_refiner_search(self._h, _ptr(Xq), nq, int(k), _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def search_device(self, d_queries, k: int, out=None):
        """search() on torch CUDA tensors (queries nq x D float32), enqueued on torch's current stream, no
        synchronisation; returns (labels nq x k int32, distances nq x k float32)."""
        import torch
        q = d_queries.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.shape[1] == self.D
        nq = q.shape[0]
        if out is not None:
            labels, dists = out
        else:
            labels = torch.empty((nq, k), dtype=torch.int32, device=q.device)
            dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        st = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check(_lib.load().vaqhip_refiner_search_device(
            self._h, C.c_void_p(q.data_ptr()), nq, int(k), C.c_void_p(labels.data_ptr()), C.c_void_p(dists.data_ptr()),
            C.c_void_p(st)))
        return labels, dists

    def last_search_timing(self) -> dict:
        t = _lib.RefinerSearchTiming()
        _lib.check(_lib.load().vaqhip_refiner_last_search_timing(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def close(self) -> None:
        if self._h:
            _lib.load().vaqhip_refiner_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VaqMultiRefiner:
    """VaqRefiner with the raw rows cut over several GPUs (vaqhip_multi_refiner_*): every shard computes the distances
    of the candidates it holds, one selection on the first device finishes -- the single refiner's answer slot for
    slot, with exact_ties on or off and for any number of shards.  `devices` as for VaqHipMulti (a device named
    several times gives logical shards on that GPU).

        r = VaqMultiRefiner([0, 1, 2, 3], D)
        r.set_rows(XTrain)                          # cut like the multi index's code rows, one upload per shard
        ans = r.refine(XTest, candidates, k)
        ans = multi.search_refine(XTest, R, k, r)   # fused with VaqHipMulti.search
        truth = r.search(XTest, k)                  # exhaustive: the true k nearest rows over all shards
    """

    def __init__(self, devices: Sequence[int], D: int):
        self.D = int(D)
        self.devices = [int(d) for d in devices]
        self._exact = False
        self._h = C.c_void_p()
        h = C.c_void_p()
        devs = (C.c_int * len(self.devices))(*self.devices)
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_create(C.byref(h), self.D, len(self.devices), devs))
        self._h = h

    def _rows(self, X) -> np.ndarray:
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.D:
            raise _lib.VaqHipError(-1, f"rows {X.shape} are not n x {self.D}")
        return X

    def set_rows(self, XTrain, id_base: int = 0) -> None:
        """Replace the rows (a host array): shard g takes rows [g * ceil(N / G), (g + 1) * ceil(N / G))."""
        X = self._rows(XTrain)
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_set_rows(self._h, _ptr(X), X.shape[0], int(id_base)))

    def add_rows(self, X) -> None:
        """Append rows; their labels continue behind the rows already held, so they extend the last shard."""
        X = self._rows(X)
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_add_rows(self._h, _ptr(X), X.shape[0]))

    def _rows_u8(self, X) -> np.ndarray:
        X = np.asarray(X)
        if X.dtype != np.uint8 or X.ndim != 2 or X.shape[1] != self.D or not X.flags.c_contiguous:
            raise _lib.VaqHipError(-1, f"byte rows must be a contiguous uint8 n x {self.D} array (nothing is converted)")
        return X

    def set_rows_u8(self, XTrain, id_base: int = 0) -> None:
        """set_rows with the rows kept as uint8 on the shards (VaqRefiner.set_rows_u8), cut as set_rows cuts."""
        X = self._rows_u8(XTrain)
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_set_rows_u8(self._h, _ptr(X), X.shape[0], int(id_base)))

    def add_rows_u8(self, X) -> None:
        """Append byte rows to byte rows (or to none): they extend the last shard.  ESTATE (-7) on float rows."""
        X = self._rows_u8(X)
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_add_rows_u8(self._h, _ptr(X), X.shape[0]))

    @property
    def elem_size(self) -> int:
        """Bytes per element of the rows held: 4 (float32) or 1 (uint8)."""
        return _lib.check_multi(_lib.load().vaqhip_multi_refiner_elem_size(self._h))

    def set_option(self, key: str, value: int) -> None:
        """"exact_ties", "timing", "exhaustive_splits" (per shard: 0 = automatic, 1..64)."""
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_set_option(self._h, key.encode(), int(value)))
        if key == "exact_ties":
            self._exact = bool(value)

    @property
    def exact_ties(self) -> bool:
        return self._exact

    @exact_ties.setter
    def exact_ties(self, on: bool) -> None:
        self.set_option("exact_ties", 1 if on else 0)
        self._exact = bool(on)

    def refine(self, XTest, answersIn, k: int) -> LabelDistVec:
        """As VaqRefiner.refine: answersIn is a LabelDistVec or an array of nq * R labels."""
        Xq = self._rows(XTest)
        nq = Xq.shape[0]
        lab = np.ascontiguousarray(getattr(answersIn, "labels", answersIn), dtype=np.int32).reshape(-1)
        R = lab.size // max(nq, 1)
        if nq and lab.size != nq * R:
            raise _lib.VaqHipError(-1, f"{lab.size} labels for {nq} queries")
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        if nq == 0:
            return ret
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_refine(self._h, _ptr(Xq), nq, _ptr(lab), R, int(k),
                                                                 _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def refine_device(self, d_queries, d_labels_in, k: int, out=None):
        """torch CUDA tensors on the FIRST device of the list in and out, enqueued behind torch's current stream of
        that device; nothing is synchronised."""
        import torch
        q = d_queries.contiguous()
        lin = d_labels_in.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.shape[1] == self.D
        assert lin.is_cuda and lin.dtype == torch.int32 and lin.shape[0] == q.shape[0]
        nq, R = lin.shape
        if out is not None:
            labels, dists = out
        else:
            labels = torch.empty((nq, k), dtype=torch.int32, device=q.device)
            dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        st = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_refine_device(
            self._h, C.c_void_p(q.data_ptr()), nq, C.c_void_p(lin.data_ptr()), R, int(k),
            C.c_void_p(labels.data_ptr()), C.c_void_p(dists.data_ptr()), C.c_void_p(st)))
        return labels, dists

    def search(self, XTest, k: int) -> LabelDistVec:
        """VaqRefiner.search over the rows of all shards: the same labels and distances slot for slot, with exact_ties
        on or off -- every shard selects over its own rows, the first device merges, and with exact_ties the queries
        that hold equal distances are replayed through the reference's heap shard after shard in row order."""
        Xq = self._rows(XTest)
        nq = Xq.shape[0]
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_search(self._h, _ptr(Xq), nq, int(k), _ptr(ret.labels),
                                                                 _ptr(ret.distances)))
        return ret

    def search_device(self, d_queries, k: int, out=None):
        """search() on torch CUDA tensors on the FIRST device of the list (queries nq x D float32), enqueued behind
        torch's current stream of that device; nothing is synchronised."""
        import torch
        q = d_queries.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.shape[1] == self.D
        nq = q.shape[0]
        if out is not None:
            labels, dists = out
        else:
            labels = torch.empty((nq, k), dtype=torch.int32, device=q.device)
            dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        st = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_search_device(
            self._h, C.c_void_p(q.data_ptr()), nq, int(k), C.c_void_p(labels.data_ptr()), C.c_void_p(dists.data_ptr()),
            C.c_void_p(st)))
        return labels, dists

    def fit_quantiles(self, bits: Sequence[int], eigvec: Optional[np.ndarray] = None):
        """vaqhip_multi_refiner_lut_fit_quantiles: binaryEncodingLUT's quantile codebooks over the RAW rows resident on
        the shards, read in place (eigvec: D x D, applied first; None: the rows are their own image).  Returns
        (cent[D, 256], q[D, 257]), bit for bit the single fit's over all rows.  Byte rows (set_rows_u8) are read as
        they lie, a byte widened where it is loaded: the fit's result over the widened rows."""
        return _fit_quantiles_call(self.D, bits, eigvec, lambda L, b, e, c, q: L.vaqhip_multi_refiner_lut_fit_quantiles(
            self._h, b, e, c, q))

    def fit_codebooks(self, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25):
        """vaqhip_multi_refiner_fit_codebooks: fit_codebooks() over the RAW rows resident on the shards, float or byte,
        read in place; subspace s is fitted on shard s % G from the columns the shards send it.  Returns what
        fit_codebooks returns, bit for bit the single fit's over all rows."""
        return _fit_codebooks_call(self.D, M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn:
                                   L.vaqhip_multi_refiner_fit_codebooks(self._h, int(M), b, e, it, c, i, nn), multi=True)

    def last_search_timing(self) -> dict:
        """Figures of the last search (times only under set_option("timing", 1)): the slowest shard's select, merge and
        link, the gather, the cross-shard merge, the flag step and the chain on the first device."""
        t = _lib.MultiRefinerSearchTiming()
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_last_search_timing(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def info(self) -> dict:
        """Shard rows, and the phase times of the last refine made under set_option("timing", 1) (waits for it)."""
        inf = _lib.MultiRefinerInfo()
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_get_info(self._h, C.byref(inf)))
        n = inf.n_devices
        d = {f: getattr(inf, f) for f, _ in _lib.MultiRefinerInfo._fields_ if f not in ("device_ids", "shard_rows")}
        d.update(device_ids=list(inf.device_ids)[:n], shard_rows=list(inf.shard_rows)[:n])
        return d

    def close(self) -> None:
        if self._h:
            _lib.load().vaqhip_multi_refiner_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fit_codebooks_call(D: int, M: int, bits, eigvec, max_iter: int, call, multi: bool = False):
    """The arrays around a vaqhip_*fit_codebooks call: ([M centre matrices k_s x L], iterations[M], nan_rows[M]).
    multi: a sharded call, whose error text is vaqhip_multi_last_error's."""
    bits = [int(b) for b in bits]
    M = int(M)
    if M < 1 or len(bits) != M or D % M != 0:
        raise _lib.VaqHipError(-1, f"{len(bits)} bits for M = {M} subspaces of D = {D}")
    eig = None
    if eigvec is not None:
        eig = np.ascontiguousarray(np.real(eigvec), dtype=np.float32)
        if eig.shape != (D, D):
            raise _lib.VaqHipError(-1, f"eigvec {eig.shape} is not {D}x{D}")
    L_ = D // M
    ks = [1 << b if 0 < b < 31 else 0 for b in bits]  # (bits out of range: the call refuses them, nothing is written)
    cent = np.empty(max(sum(ks) * L_, 1), np.float32)
    iters = np.zeros(M, np.int32)
    nan_rows = np.zeros(M, np.int32)
    (_lib.check_multi if multi else _lib.check)(call(_lib.load(), (C.c_int * M)(*bits), _ptr(eig) if eig is not None else None,
                                                     int(max_iter), _ptr(cent), _ptr(iters), _ptr(nan_rows)))
    offs = np.concatenate([[0], np.cumsum(ks)]) * L_
    return [cent[offs[s]:offs[s + 1]].reshape(ks[s], L_).copy() for s in range(M)], iters, nan_rows


def _fit_codebooks_sharded(fn_name: str, devices, X, M, bits, eigvec, max_iter):
    devs = [int(d) for d in devices]
    arr = (C.c_int * max(len(devs), 1))(*devs)
    return _fit_codebooks_call(X.shape[1], M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: getattr(L, fn_name)(
        len(devs), arr, _ptr(X), X.shape[0], X.shape[1], int(M), b, e, it, c, i, nn), multi=True)


def fit_codebooks(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25, device: int = 0,
                  devices: Optional[Sequence[int]] = None):
    """vaqhip_fit_codebooks: the subspace codebooks mCentroidsPerSubs by KMeans::staticFitSampling (the call of
    VAQ.cpp:644-649; not the arma::kmeans call VAQ::train runs today), every subspace fitted on the device, bit for
    bit the reference's.  X: n x D rows (unprojected when eigvec is given, else in PCA space); bits[M].  Returns
    ([M arrays (1 << bits[s]) x L], iterations[M], nan_rows[M]).  devices=[...]: the same result from the sharded fit
    (vaqhip_multi_fit_codebooks): the rows are cut over the devices, subspace s is fitted on devices[s % G] and no
    device holds all rows; a device named several times gives logical shards on that GPU."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise _lib.VaqHipError(-1, f"X {X.shape} is not n x D")
    if devices is not None:
        return _fit_codebooks_sharded("vaqhip_multi_fit_codebooks", devices, X, M, bits, eigvec, max_iter)
    return _fit_codebooks_call(X.shape[1], M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: L.vaqhip_fit_codebooks(
        int(device), _ptr(X), X.shape[0], X.shape[1], int(M), b, e, it, c, i, nn))


def fit_codebooks_u8(X, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25, device: int = 0,
                     devices: Optional[Sequence[int]] = None):
    """fit_codebooks from byte rows (vaqhip_fit_codebooks_u8, or vaqhip_multi_fit_codebooks_u8 with devices): the result
    is fit_codebooks's on X.astype(float32), bit for bit.  Anything but a contiguous uint8 n x D array is EINVAL."""
    X = np.asarray(X)
    X = _u8_rows(X, X.shape[1] if X.ndim == 2 else 0)
    if devices is not None:
        return _fit_codebooks_sharded("vaqhip_multi_fit_codebooks_u8", devices, X, M, bits, eigvec, max_iter)
    return _fit_codebooks_call(X.shape[1], M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: L.vaqhip_fit_codebooks_u8(
        int(device), _ptr(X), X.shape[0], X.shape[1], int(M), b, e, it, c, i, nn))


def fit_codebooks_timing(on: bool) -> None:
    """Phase times for the calling thread's fits (vaqhip_fit_codebooks_set_timing): one synchronisation per phase."""
    _lib.check(_lib.load().vaqhip_fit_codebooks_set_timing(1 if on else 0))


def last_fit_codebooks_timing() -> dict:
    """Figures of the calling thread's last codebook fit (vaqhip_last_fit_codebooks_timing)."""
    t = _lib.FitCodebooksTiming()
    _lib.check(_lib.load().vaqhip_last_fit_codebooks_timing(C.byref(t)))
    return {f: getattr(t, f) for f, _ in _lib.FitCodebooksTiming._fields_}


def last_multi_fit_codebooks_timing() -> dict:
    """Figures of the calling thread's last sharded codebook fit (vaqhip_multi_last_fit_codebooks_timing); the owners'
    assign / accumulate / update times only under fit_codebooks_timing(True)."""
    t = _lib.MultiFitCodebooksTiming()
    _lib.check_multi(_lib.load().vaqhip_multi_last_fit_codebooks_timing(C.byref(t)))
    d = {f: getattr(t, f) for f, _ in _lib.MultiFitCodebooksTiming._fields_ if f != "owner_subspaces"}
    d["owner_subspaces"] = list(t.owner_subspaces)[:t.n_devices]
    return d


def _fit_quantiles_call(D: int, bits, eigvec, call):
    bits = [int(b) for b in bits]
    if len(bits) != D:
        raise _lib.VaqHipError(-1, f"{len(bits)} bits for D = {D}")
    eig = None
    if eigvec is not None:
        eig = np.ascontiguousarray(np.real(eigvec), dtype=np.float32)
        if eig.shape != (D, D):
            raise _lib.VaqHipError(-1, f"eigvec {eig.shape} is not {D}x{D}")
    cent = np.empty((D, 256), np.float32)
    q = np.empty((D, 257), np.float32)
    _lib.check_multi(call(_lib.load(), (C.c_int * max(D, 1))(*bits), _ptr(eig) if eig is not None else None, _ptr(cent),
                          _ptr(q)))
    return cent, q


def lut_fit_quantiles_multi(devices: Sequence[int], X, bits: Sequence[int], eigvec: Optional[np.ndarray] = None):
    """vaqhip_multi_lut_fit_quantiles: vaqhip_lut_fit_quantiles's (cent[D, 256], q[D, 257]) bit for bit, with the rows
    of X cut over `devices` as VaqHipMulti.set_codes cuts code rows and dimension d fitted on device d % len(devices);
    no device holds all rows.  A device named several times gives logical shards on that GPU."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise _lib.VaqHipError(-1, f"X {X.shape} is not n x D")
    devs = [int(d) for d in devices]
    arr = (C.c_int * max(len(devs), 1))(*devs)
    return _fit_quantiles_call(X.shape[1], bits, eigvec, lambda L, b, e, c, q: L.vaqhip_multi_lut_fit_quantiles(
        len(devs), arr, _ptr(X), X.shape[0], X.shape[1], b, e, c, q))


def lut_fit_quantiles_multi_u8(devices: Sequence[int], X, bits: Sequence[int], eigvec: Optional[np.ndarray] = None):
    """lut_fit_quantiles_multi from byte rows (vaqhip_multi_lut_fit_quantiles_u8): every shard uploads its slice as
    n_g x D bytes; the result is lut_fit_quantiles_multi's on X.astype(float32), bit for bit.  Anything but a
    contiguous uint8 n x D array is EINVAL."""
    X = np.asarray(X)
    X = _u8_rows(X, X.shape[1] if X.ndim == 2 else 0)
    devs = [int(d) for d in devices]
    arr = (C.c_int * max(len(devs), 1))(*devs)
    return _fit_quantiles_call(X.shape[1], bits, eigvec, lambda L, b, e, c, q: L.vaqhip_multi_lut_fit_quantiles_u8(
        len(devs), arr, _ptr(X), X.shape[0], X.shape[1], b, e, c, q))


def last_lut_fit_multi_timing() -> dict:
    """Figures of the calling thread's last sharded fit (vaqhip_multi_last_lut_fit_timing)."""
    t = _lib.MultiLutFitTiming()
    _lib.check_multi(_lib.load().vaqhip_multi_last_lut_fit_timing(C.byref(t)))
    return {f: getattr(t, f) for f, _ in _lib.MultiLutFitTiming._fields_}


def merge_topk_device(dist_lists, label_lists, k: int, out=None):
    """Multi-GPU exchange step: [n_lists, nq, k] CUDA tensors (labels global,
    empty slots -1 / FLT_MAX) -> per-query k smallest by (distance, label)."""
    import torch
    d = dist_lists.contiguous()
    l = label_lists.contiguous()
    n_lists, nq, kk = d.shape
    assert kk == k and l.shape == d.shape and l.dtype == torch.int32 and d.dtype == torch.float32
    if out is not None:
        out_l, out_d = out
    else:
        out_l = torch.empty((nq, k), dtype=torch.int32, device=d.device)
        out_d = torch.empty((nq, k), dtype=torch.float32, device=d.device)
    st = torch.cuda.current_stream(d.device).cuda_stream
    dev = d.device.index if d.device.index is not None else torch.cuda.current_device()
    _lib.check(_lib.load().vaqhip_merge_topk_device(
        dev, C.c_void_p(d.data_ptr()), C.c_void_p(l.data_ptr()), n_lists, nq, k,
        C.c_void_p(out_l.data_ptr()), C.c_void_p(out_d.data_ptr()), C.c_void_p(st)))
    return out_l, out_d


def merge_topk_packed_device(packed, world: int, nq: int, k: int, out=None):
    """packed: int32 CUDA tensor [world, 2, nq, k] from ONE all-gather -- plane 0 holds
    labels, plane 1 the float32 distance bits.  Returns the merged (labels, distances)."""
    import torch
    assert packed.is_contiguous() and packed.dtype == torch.int32 and packed.numel() == world * 2 * nq * k
    if out is not None:
        out_l, out_d = out
    else:
        out_l = torch.empty((nq, k), dtype=torch.int32, device=packed.device)
        out_d = torch.empty((nq, k), dtype=torch.float32, device=packed.device)
    st = torch.cuda.current_stream(packed.device).cuda_stream
    dev = packed.device.index if packed.device.index is not None else torch.cuda.current_device()
    base = packed.data_ptr()
    _lib.check(_lib.load().vaqhip_merge_topk_strided_device(
        dev, C.c_void_p(base + nq * k * 4), C.c_void_p(base), world, 2 * nq * k, k, nq, k,
        C.c_void_p(out_l.data_ptr()), C.c_void_p(out_d.data_ptr()), C.c_void_p(st)))
    return out_l, out_d


def merge_fast_device(head_dist, dist_lists, label_lists, k: int, head_label_base: int = 0, out=None):
    """FAST's exchange step (vaqhip_merge_fast_device): head_dist uint16-valued int16 CUDA tensor [nq, n_head]
    -- the distances of the first n_head = min(k, N) rows of the whole database -- and [n_lists, nq, k] lists of
    the OTHER rows, each ascending by (distance, row), lists in row order, empty slots -1 / FLT_MAX.  Returns the
    single index's FAST answer: the first k of the stable merge by distance of the head in std::sort's order,
    then the lists."""
    import torch
    d = dist_lists.contiguous()
    l = label_lists.contiguous()
    h = head_dist.contiguous()
    n_lists, nq, kk = d.shape
    assert kk == k and l.shape == d.shape and l.dtype == torch.int32 and d.dtype == torch.float32
    assert h.dim() == 2 and h.shape[0] == nq and h.element_size() == 2 and h.shape[1] <= k
    if out is not None:
        out_l, out_d = out
    else:
        out_l = torch.empty((nq, k), dtype=torch.int32, device=d.device)
        out_d = torch.empty((nq, k), dtype=torch.float32, device=d.device)
    st = torch.cuda.current_stream(d.device).cuda_stream
    dev = d.device.index if d.device.index is not None else torch.cuda.current_device()
    _lib.check(_lib.load().vaqhip_merge_fast_device(
        dev, C.c_void_p(h.data_ptr()), h.shape[1], h.shape[1], int(head_label_base), C.c_void_p(d.data_ptr()),
        C.c_void_p(l.data_ptr()), n_lists, nq * k, k, nq, k, C.c_void_p(out_l.data_ptr()),
        C.c_void_p(out_d.data_ptr()), C.c_void_p(st)))
    return out_l, out_d


class VaqHipMulti:
    """One process, several GPUs (include/vaqhip.h "multi-device"): the rows are sharded
    contiguously over `devices`, every device answers all queries on its shard, one RCCL
    all-gather + merge finishes the search.  Naming a device several times gives logical shards
    on that GPU (gather by device copies) -- the form a one-GPU box can test."""

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
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.D:
            raise _lib.VaqHipError(-1, f"rows {X.shape} are not n x {self.D}")
        return X

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
        codes = None
        if return_codes:
            codes = np.empty((refiner.info()["N"], self.M), np.uint16)
        _lib.check_multi(_lib.load().vaqhip_multi_encode_from_refiner(self._h, refiner._h,
                                                                      _ptr(codes) if return_codes else None))
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
        codes = None
        if return_codes:
            codes = np.empty((refiner.info()["N"], self.M), np.uint16)
        _lib.check_multi(_lib.load().vaqhip_multi_encode_lut_from_refiner(self._h, refiner._h,
                                                                          _ptr(codes) if return_codes else None))
        return codes

    def last_encode_timing(self) -> dict:
        t = _lib.MultiEncodeTiming()
        _lib.check_multi(_lib.load().vaqhip_multi_last_encode_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in _lib.MultiEncodeTiming._fields_}

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
        X = np.ascontiguousarray(XTrain, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.D:
            raise _lib.VaqHipError(-1, f"XTrain {X.shape} is not n x {self.D}")
        off = np.empty(self.M, np.float32)
        sc = np.empty(self.M, np.float32)
        _lib.check_multi(_lib.load().vaqhip_multi_learn_quantization(
            self._h, _ptr(X), X.shape[0], 1 if projected else 0, C.c_float(sampleRatio), _ptr(off), _ptr(sc)))
        return off, sc

    def learn_quantization_u8(self, XTrain: np.ndarray, sampleRatio: float, projected: bool = False):
        """learn_quantization() from byte rows (vaqhip_multi_learn_quantization_u8); anything but a contiguous uint8
        n x D array is EINVAL.  Returns (offsets, scale)."""
        X = _u8_rows(XTrain, self.D)
        off = np.empty(self.M, np.float32)
        sc = np.empty(self.M, np.float32)
        _lib.check_multi(_lib.load().vaqhip_multi_learn_quantization_u8(
            self._h, _ptr(X), X.shape[0], 1 if projected else 0, C.c_float(sampleRatio), _ptr(off), _ptr(sc)))
        return off, sc

    def learn_quantization_from_refiner(self, refiner: "VaqMultiRefiner", sampleRatio: float):
        """learn_quantization() over the raw rows a VaqMultiRefiner on the same devices holds, read where they are
        (vaqhip_multi_learn_quantization_from_refiner).  Returns (offsets, scale)."""
        off = np.empty(self.M, np.float32)
        sc = np.empty(self.M, np.float32)
        _lib.check_multi(_lib.load().vaqhip_multi_learn_quantization_from_refiner(
            self._h, refiner._h, C.c_float(sampleRatio), _ptr(off), _ptr(sc)))
        return off, sc

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
        return {f: getattr(t, f) for f, _ in _lib.KmeansTiming._fields_}

    def search(self, XTest: np.ndarray, k: int, projected: bool = False) -> LabelDistVec:
        X = np.ascontiguousarray(XTest, dtype=np.float32)
        nq = X.shape[0]
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        _lib.check_multi(_lib.load().vaqhip_multi_search(self._h, _ptr(X), nq, k, 1 if projected else 0,
                                                         _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def search_device(self, d_queries, k: int, projected: bool = False, out=None):
        """vaqhip_multi_search_device: torch CUDA tensors on the FIRST device of the list in and out,
        enqueued behind torch's current stream of that device; nothing is synchronised."""
        import torch
        q = d_queries.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.shape[1] == self.D
        nq = q.shape[0]
        if out is None:
            out = (torch.empty((nq, k), dtype=torch.int32, device=q.device),
                   torch.empty((nq, k), dtype=torch.float32, device=q.device))
        labels, dists = out
        stream = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check_multi(_lib.load().vaqhip_multi_search_device(
            self._h, C.c_void_p(q.data_ptr()), nq, k, 1 if projected else 0, C.c_void_p(labels.data_ptr()),
            C.c_void_p(dists.data_ptr()), C.c_void_p(stream)))
        return labels, dists

    def search_refine(self, XTest: np.ndarray, R: int, k: int, refiner: "VaqMultiRefiner") -> LabelDistVec:
        """search(XTest, R) followed by VAQ::refine to k against the multi refiner's sharded rows, in one call
        (vaqhip_multi_search_refine): the candidates go from the merge on the first device straight into the refine.
        Equals search() + refiner.refine() on the same inputs; this index's options apply to the search half."""
        X = np.ascontiguousarray(XTest, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.D:
            raise _lib.VaqHipError(-1, f"XTest {X.shape} is not nq x {self.D}")
        nq = X.shape[0]
        ret = LabelDistVec(np.empty(nq * k, np.int32), np.empty(nq * k, np.float32))
        _lib.check_multi(_lib.load().vaqhip_multi_search_refine(self._h, refiner._h, _ptr(X), nq, int(R), int(k),
                                                                _ptr(ret.labels), _ptr(ret.distances)))
        return ret

    def search_refine_device(self, d_queries, R: int, k: int, refiner: "VaqMultiRefiner", out=None):
        """vaqhip_multi_search_refine_device: torch CUDA tensors on the first device, enqueue only."""
        import torch
        q = d_queries.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.shape[1] == self.D
        nq = q.shape[0]
        if out is None:
            out = (torch.empty((nq, k), dtype=torch.int32, device=q.device),
                   torch.empty((nq, k), dtype=torch.float32, device=q.device))
        labels, dists = out
        stream = torch.cuda.current_stream(q.device).cuda_stream
        _lib.check_multi(_lib.load().vaqhip_multi_search_refine_device(
            self._h, refiner._h, C.c_void_p(q.data_ptr()), nq, int(R), int(k), C.c_void_p(labels.data_ptr()),
            C.c_void_p(dists.data_ptr()), C.c_void_p(stream)))
        return labels, dists

    def shard(self, g: int):
        """vaqhip_multi_shard: the raw handle of shard g's single-device index (owned by the multi index)."""
        return _lib.load().vaqhip_multi_shard(self._h, g)

    def info(self) -> dict:
        inf = _lib.MultiInfo()
        _lib.check_multi(_lib.load().vaqhip_multi_get_info(self._h, C.byref(inf)))
        n = inf.n_devices
        return dict(n_devices=n, exchange=inf.exchange, N=inf.N, id_base=inf.id_base,
                    device_ids=list(inf.device_ids)[:n], shard_rows=list(inf.shard_rows)[:n],
                    last_search_ms=inf.last_search_ms, last_exchange_ms=inf.last_exchange_ms,
                    last_merge_ms=inf.last_merge_ms)

    def close(self) -> None:
        if self._h:
            _lib.load().vaqhip_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VaqHipFast(VaqHip):
    """VAQ with the FAST search method (VAQ::searchFast, VAQ.cpp:1778-1834): every
    table is quantised to uint8 by mOffsets / mScale (smallQuantize), rows are
    summed as integers and the k best are KNNFromDists' choice, slot for slot
    (include/vaqhip.h, vaqhip_index_set_lut_quantization).  Codes of at most 4
    bits (mMaxBitsPerSubs <= 4).  Method precedence is the reference's:
    TI > EA > HEAP > FAST.

    Typical use (mirrors demo_vaq.cpp:120-124)::

        vaq = VaqHipFast()
        vaq.parseMethodString("VAQ256m64min4max4var1,FAST")
        ...                                    # mBitsAlloc, mCentroidsPerSubs, mEigenVectors
        vaq.encode(XTrainPCA)                  # mCodebook and mCodebookCMajor
        vaq.learnQuantization(XTrain, 0.1)     # mOffsets, mScale
        ans = vaq.search(XTest, 100)
    """

    _METHODS = VaqHip._METHODS | NNMethod.Fast

    def __init__(self, device: int = 0):
        super().__init__(device=device)
        self.mOffsets: Optional[np.ndarray] = None  # [M] float32 (VAQ.hpp: RowVector<float>)
        self.mScale: Optional[np.ndarray] = None    # [M] float32 (VAQ.hpp: ColVector<float>)
        self.mCodebookCMajor: Optional[np.ndarray] = None
        self._q_sig = None

    def parseMethodString(self, methodString: str) -> None:
        """VAQ::parseMethodString with FAST accepted, and the reference's check
        after it (VAQ.cpp:1263-1266): FAST with mMaxBitsPerSubs > 4 is refused
        (the reference exits; here VaqHipError EUNSUPPORTED)."""
        super().parseMethodString(methodString)
        if (self.mMethods & NNMethod.Fast) and self.mMaxBitsPerSubs > 4:
            raise _lib.VaqHipError(-2, "max bit per subs couldn't be > 4 when using FAST query method "
                                       f"(max {self.mMaxBitsPerSubs})")

    # ----------------------------------------------------------- quantisation --
    def setLUTQuantization(self, offsets, scale) -> None:
        """mOffsets / mScale, checked as vaqhip_index_set_lut_quantization checks
        them: M finite values each, every scale > 0."""
        off = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1)
        sc = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        M = len(self.mBitsAlloc)
        if M and (off.shape[0] != M or sc.shape[0] != M):
            raise _lib.VaqHipError(-1, f"offsets {off.shape} / scale {sc.shape}: need {M} values each")
        if off.shape != sc.shape:
            raise _lib.VaqHipError(-1, f"offsets {off.shape} and scale {sc.shape} differ in length")
        if not (np.all(np.isfinite(off)) and np.all(np.isfinite(sc)) and np.all(sc > 0)):
            raise _lib.VaqHipError(-1, "offsets and scale must be finite and every scale > 0")
        self.mOffsets = off
        self.mScale = sc

    def learnQuantization(self, XTrain: np.ndarray, sampleRatio: float, projected: bool = False) -> None:
        """VAQ::learnQuantization (VAQ.cpp:1118-1187) on the GPU tables:
        sets mOffsets / mScale.  XTrain is unprojected unless projected=True."""
        X = np.ascontiguousarray(XTrain, dtype=np.float32)
        if X.ndim != 2:
            raise _lib.VaqHipError(-1, f"XTrain {X.shape} is not n x D")
        if int(np.float32(sampleRatio) * np.float32(X.shape[0])) < 1:
            raise _lib.VaqHipError(-1, f"sampleSize = int({sampleRatio} * {X.shape[0]}) < 1")
        self._ensure_index()
        if X.shape[1] != self.mTotalDim:
            raise _lib.VaqHipError(-1, f"XTrain {X.shape} is not n x {self.mTotalDim}")
        M = len(self.mBitsAlloc)
        off = np.empty(M, np.float32)
        sc = np.empty(M, np.float32)
        _lib.check(_lib.load().vaqhip_learn_quantization(self._h, _ptr(X), X.shape[0], 1 if projected else 0,
                                                         C.c_float(sampleRatio), _ptr(off), _ptr(sc)))
        self.mOffsets, self.mScale = off, sc
        self._q_sig = (self._h.value, _wref(off), _wref(sc))

    def _learn_with(self, call) -> None:
        """One of the device forms: call(off, sc) -> code; mOffsets / mScale on success, as learnQuantization."""
        M = len(self.mBitsAlloc)
        off = np.empty(M, np.float32)
        sc = np.empty(M, np.float32)
        _lib.check(call(_ptr(off), _ptr(sc)))
        self.mOffsets, self.mScale = off, sc
        self._q_sig = (self._h.value, _wref(off), _wref(sc))

    def learnQuantization_u8(self, XTrain: np.ndarray, sampleRatio: float, projected: bool = False) -> None:
        """learnQuantization() from byte rows (vaqhip_learn_quantization_u8): only the sampled rows are uploaded, as
        bytes; mOffsets / mScale are those of learnQuantization(XTrain.astype(float32)), bit for bit.  Anything but
        a contiguous uint8 n x D array is EINVAL: nothing is converted."""
        X = _u8_rows(XTrain, self.mTotalDim)
        self._ensure_index()
        self._learn_with(lambda off, sc: _lib.load().vaqhip_learn_quantization_u8(
            self._h, _ptr(X), X.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

    def learnQuantization_device(self, d_X, sampleRatio: float, projected: bool = False) -> None:
        """learnQuantization() from a float32 torch CUDA tensor on the index's device
        (vaqhip_learn_quantization_device).  The call runs on the index's own stream: torch's current stream is
        synchronised first, so that the rows are complete."""
        import torch
        x = d_X.contiguous()
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.mTotalDim):
            raise _lib.VaqHipError(-1, f"rows must be a float32 n x {self.mTotalDim} CUDA tensor")
        self._ensure_index()
        torch.cuda.current_stream(x.device).synchronize()
        self._learn_with(lambda off, sc: _lib.load().vaqhip_learn_quantization_device(
            self._h, C.c_void_p(x.data_ptr()), x.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

    def learnQuantization_u8_device(self, d_X, sampleRatio: float, projected: bool = False) -> None:
        """The same from a uint8 torch CUDA tensor (vaqhip_learn_quantization_u8_device); it may start at any byte."""
        import torch
        x = _u8_rows_device(d_X, self.mTotalDim)
        self._ensure_index()
        torch.cuda.current_stream(x.device).synchronize()
        self._learn_with(lambda off, sc: _lib.load().vaqhip_learn_quantization_u8_device(
            self._h, C.c_void_p(x.data_ptr()), x.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

    def learnQuantizationFromRefiner(self, refiner: "VaqRefiner", sampleRatio: float) -> None:
        """learnQuantization() over the raw rows resident in a VaqRefiner on the same device, float or byte, read in
        place (vaqhip_learn_quantization_from_refiner)."""
        self._ensure_index()
        self._learn_with(lambda off, sc: _lib.load().vaqhip_learn_quantization_from_refiner(
            self._h, refiner._h, C.c_float(sampleRatio), off, sc))

    def _ensure_quant(self):
        if self.mOffsets is None or self.mScale is None:
            return  # a FAST search then reports the missing quantisation (ESTATE)
        if (self._q_sig is not None and self._q_sig[0] == self._h.value
                and _same(self._q_sig[1], self.mOffsets) and _same(self._q_sig[2], self.mScale)):
            return
        self.setLUTQuantization(self.mOffsets, self.mScale)
        _lib.check(_lib.load().vaqhip_index_set_lut_quantization(self._h, _ptr(self.mOffsets), _ptr(self.mScale)))
        self._q_sig = (self._h.value, _wref(self.mOffsets), _wref(self.mScale))

    def _ensure_codes(self):
        super()._ensure_codes()
        self._ensure_quant()

    def close(self) -> None:
        super().close()
        self._q_sig = None  # a new index starts without a quantisation

    # -------------------------------------------------------------- codes --
    def encode(self, XTrain: np.ndarray, projected: bool = True) -> None:
        """VAQ::encode; FAST also keeps the codes as mCodebookCMajor (uint8,
        column-major, rows padded to 32 with code 0, VAQ.cpp:666-670, 718)."""
        super().encode(XTrain, projected=projected)
        N, M = self.mCodebook.shape
        n_pad = (N + 31) // 32 * 32
        cm = np.zeros((n_pad, M), np.uint8, order="F")
        cm[:N] = self.mCodebook
        self.mCodebookCMajor = cm

    def buildSmallLUT(self, XTest: np.ndarray, projected: bool = False) -> np.ndarray:
        """smallQuantize(CreateLUT(query)) for every query: (nq, M, 16) uint8
        (vaqhip_build_small_lut; entries past 1 << max(bits) are 0)."""
        self._ensure_index()
        self._ensure_quant()
        X = np.ascontiguousarray(XTest, dtype=np.float32)
        out = np.empty((X.shape[0], len(self.mBitsAlloc), 16), np.uint8)
        _lib.check(_lib.load().vaqhip_build_small_lut(self._h, _ptr(X), X.shape[0], 1 if projected else 0,
                                                      _ptr(out)))
        return out
