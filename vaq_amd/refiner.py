"""VaqRefiner and VaqMultiRefiner: the raw rows VAQ::refine reads, resident on one device or cut over several, over
vaqhip_refiner_* and vaqhip_multi_refiner_*.  The two C families take the same arguments call for call, so one base
class holds every method they share; a subclass names its symbol prefix, its error check and its timing structure,
and adds what only it has."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._adapt import _Handle, _dptr, _f32_rows, _out_pair, _ptr, _stream, _struct_dict, _u8_rows
from .fits import _check_fittable, _fit_codebooks_call, _fit_quantiles_call, _train_rotation_call
from .single import LabelDistVec, _new_answer


class _RefinerBase(_Handle):
    """What VaqRefiner and VaqMultiRefiner share.  _prefix + name is the C symbol, _check raises with the text of
    that family's last error."""
    _prefix = ""
    _check = staticmethod(_lib.check)
    _Timing = None

    def _call(self, name: str, *args) -> int:
        return self._check(getattr(_lib.load(), self._prefix + name)(self._h, *args))

    def _rows(self, X) -> np.ndarray:
        return _f32_rows(X, self.D, "rows {shape} are not n x {D}")

    def _rows_u8(self, X) -> np.ndarray:
        return _u8_rows(X, self.D)

    def set_rows(self, XTrain, id_base: int = 0) -> None:
        """Replace the rows by a host array; row i has label id_base + i.  On several devices shard g takes rows
        [g * ceil(N / G), (g + 1) * ceil(N / G))."""
        X = self._rows(XTrain)
        self._call("set_rows", _ptr(X), X.shape[0], int(id_base))

    def add_rows(self, X) -> None:
        """Append rows; their labels continue behind the rows already held (on several devices they extend the last
        shard)."""
        X = self._rows(X)
        self._call("add_rows", _ptr(X), X.shape[0])

    def set_rows_u8(self, XTrain, id_base: int = 0) -> None:
        """Replace the rows by BYTE rows, kept as uint8 on the device (a bvecs dataset as stored): a contiguous np.uint8
        n x D array, cut as set_rows cuts.  Every call that reads the rows answers as over XTrain.astype(float32), bit
        for bit.  set_rows(uint8 array) still widens to float."""
        X = self._rows_u8(XTrain)
        self._call("set_rows_u8", _ptr(X), X.shape[0], int(id_base))

    def add_rows_u8(self, X) -> None:
        """Append byte rows to byte rows (or to none); ESTATE (-7) on float rows, as add_rows on byte rows."""
        X = self._rows_u8(X)
        self._call("add_rows_u8", _ptr(X), X.shape[0])

    @property
    def elem_size(self) -> int:
        """Bytes per element of the rows held: 4 (float32) or 1 (uint8)."""
        return self._call("elem_size")

    def fit_codebooks(self, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25):
        """fit_codebooks() over the RAW rows held, float or byte, read where they are (vaqhip_refiner_fit_codebooks;
        vaqhip_multi_refiner_fit_codebooks: subspace s is fitted on shard s % G from the columns the shards send it).
        Returns what fit_codebooks returns, bit for bit the single fit's over all rows."""
        fn = self._prefix + "fit_codebooks"
        return _fit_codebooks_call(self.D, M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: getattr(L, fn)(
            self._h, int(M), b, e, it, c, i, nn), multi=self._check is _lib.check_multi)

    def set_option(self, key: str, value: int) -> None:
        """"exact_ties", "exhaustive_splits" (per shard; 0 = automatic, 1..64), "timing"."""
        self._call("set_option", key.encode(), int(value))
        if key == "exact_ties":
            self._exact = bool(value)

    @property
    def exact_ties(self) -> bool:
        return self._exact

    @exact_ties.setter
    def exact_ties(self, on: bool) -> None:
        self.set_option("exact_ties", 1 if on else 0)

    def refine(self, XTest, answersIn, k: int) -> LabelDistVec:
        """answersIn: a LabelDistVec (as search() returns it) or an array of nq * R labels.  Labels that are negative
        or name no resident row are skipped."""
        Xq = self._rows(XTest)
        nq = Xq.shape[0]
        lab = np.ascontiguousarray(getattr(answersIn, "labels", answersIn), dtype=np.int32).reshape(-1)
        R = lab.size // max(nq, 1)
        if nq and lab.size != nq * R:
            raise _lib.VaqHipError(-1, f"{lab.size} labels for {nq} queries")
        ret = _new_answer(nq * k)
        if nq == 0:
            return ret
        self._call("refine", _ptr(Xq), nq, _ptr(lab), R, int(k), _ptr(ret.labels), _ptr(ret.distances))
        return ret

    def _queries_device(self, d_queries):
        import torch
        q = d_queries.contiguous()
        assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.shape[1] == self.D
        return q

    def refine_device(self, d_queries, d_labels_in, k: int, out=None):
        """torch CUDA tensors in and out (queries nq x D float32, labels nq x R int32; on several devices they lie on
        the FIRST device of the list), enqueued on torch's current stream of that device, no synchronisation."""
        import torch
        q = self._queries_device(d_queries)
        lin = d_labels_in.contiguous()
        assert lin.is_cuda and lin.dtype == torch.int32 and lin.shape[0] == q.shape[0]
        nq, R = lin.shape
        labels, dists = _out_pair(out, nq, k, q.device)
        self._call("refine_device", _dptr(q), nq, _dptr(lin), R, int(k), _dptr(labels), _dptr(dists), _stream(q))
        return labels, dists

    def search(self, XTest, k: int) -> LabelDistVec:
        """The exhaustive form of refine(): the candidates are ALL resident rows in row order -- the true k nearest rows
        of every query with the reference's own distances (and, with exact_ties, its heap's choice among equal ones).
        Over several shards the answer is the single refiner's slot for slot: every shard selects over its own rows,
        the first device merges, and with exact_ties the queries that hold equal distances are replayed through the
        reference's heap shard after shard in row order."""
        Xq = self._rows(XTest)
        nq = Xq.shape[0]
        ret = _new_answer(nq * k)
        self._call("search", _ptr(Xq), nq, int(k), _ptr(ret.labels), _ptr(ret.distances))
        return ret

    def search_device(self, d_queries, k: int, out=None):
        """search() on torch CUDA tensors (queries nq x D float32; on several devices on the FIRST device of the list),
        enqueued on torch's current stream of that device, no synchronisation; returns (labels nq x k int32,
        distances nq x k float32)."""
        q = self._queries_device(d_queries)
        nq = q.shape[0]
        labels, dists = _out_pair(out, nq, k, q.device)
        self._call("search_device", _dptr(q), nq, int(k), _dptr(labels), _dptr(dists), _stream(q))
        return labels, dists

    def last_search_timing(self) -> dict:
        """Figures of the last search (times only under set_option("timing", 1)); over several shards the slowest
        shard's select, merge and link, the gather, the cross-shard merge, the flag step and the chain on the first
        device."""
        t = self._Timing()
        self._call("last_search_timing", C.byref(t))
        return _struct_dict(t)


class VaqRefiner(_RefinerBase):
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
    _prefix = "vaqhip_refiner_"
    _destroy = "vaqhip_refiner_destroy"
    _Timing = _lib.RefinerSearchTiming

    def __init__(self, D: int, device: int = 0):
        self.D = int(D)
        self.device = device
        self._exact = False
        self._h = C.c_void_p()
        h = C.c_void_p()
        _lib.check(_lib.load().vaqhip_refiner_create(C.byref(h), device, self.D))
        self._h = h

    def _set_rows_device(self, name: str, x, dtype, id_base: int) -> None:
        import torch
        want = getattr(torch, dtype)
        if not (x.is_cuda and x.device.index == self.device and x.dtype == want and x.is_contiguous()
                and x.dim() == 2 and x.shape[1] == self.D):
            raise _lib.VaqHipError(-1, f"device rows must be a contiguous {dtype} n x {self.D} tensor on cuda:{self.device}")
        self._call(name, _dptr(x), x.shape[0], int(id_base), _stream(x))

    def set_rows(self, XTrain, id_base: int = 0) -> None:
        """Replace the rows: a host array, or a contiguous float32 torch tensor on the refiner's device (copied)."""
        if hasattr(XTrain, "data_ptr"):
            return self._set_rows_device("set_rows_device", XTrain, "float32", id_base)
        super().set_rows(XTrain, id_base)

    def set_rows_u8(self, XTrain, id_base: int = 0) -> None:
        """_RefinerBase.set_rows_u8, or from a contiguous torch.uint8 tensor on the refiner's device (copied)."""
        if hasattr(XTrain, "data_ptr"):
            return self._set_rows_device("set_rows_u8_device", XTrain, "uint8", id_base)
        super().set_rows_u8(XTrain, id_base)

    def train_moment(self):
        """The second moment of the sampled resident rows (vaqhip_refiner_train_moment): (float64 D x D, its float32
        rounding)."""
        cov, cov_f = np.empty((self.D, self.D), np.float64), np.empty((self.D, self.D), np.float32)
        self._call("train_moment", _ptr(cov), _ptr(cov_f))
        return cov, cov_f

    def train_rotation(self, M: int, bit_budget: int, min_bits: int, max_bits: int, percent_var: float = 1.0):
        """train_rotation() over the RAW rows held, float or byte, read where they are (vaqhip_refiner_train_rotation):
        what train_rotation returns on the same rows, bit for bit."""
        return _train_rotation_call(self.D, M, lambda L, e, v, b, h: L.vaqhip_refiner_train_rotation(
            self._h, int(M), int(bit_budget), int(min_bits), int(max_bits), float(percent_var), e, v, b, h))

    def _fit_codebooks_form(self, form: str, M, bits, eigvec, max_iter):
        """A wide form of the fit ("hier" or "bin") over the rows held: vaqhip_refiner_fit_codebooks_<form>."""
        fn = "vaqhip_refiner_fit_codebooks_" + form
        return _fit_codebooks_call(self.D, M, bits, eigvec, max_iter, lambda L, b, e, it, c, i, nn: getattr(L, fn)(
            self._h, int(M), b, e, it, c, i, nn))

    def fit_codebooks_hier(self, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25):
        """fit_codebooks_hier() over the RAW rows held, float or byte, read where they are
        (vaqhip_refiner_fit_codebooks_hier): subspaces above 8 bits in two stages.  Single device only."""
        return self._fit_codebooks_form("hier", M, bits, eigvec, max_iter)

    def fit_codebooks_bin(self, M: int, bits: Sequence[int], eigvec: Optional[np.ndarray] = None, max_iter: int = 25):
        """fit_codebooks_bin() over the RAW rows held, float or byte, read where they are
        (vaqhip_refiner_fit_codebooks_bin): subspaces above 8 bits as a tree of 2-centre fits.  Single device only."""
        return self._fit_codebooks_form("bin", M, bits, eigvec, max_iter)

    def train(self, M: int, bit_budget: int, min_bits: int, max_bits: int, percent_var: float = 1.0, max_iter: int = 25):
        """train_rotation() then fit_codebooks() over the rows held: (eigvec, bits, centroids), as vaq_amd.train."""
        eig, _, bits, hi = self.train_rotation(M, bit_budget, min_bits, max_bits, percent_var)
        _check_fittable(M, bits, hi)
        cents, _, _ = self.fit_codebooks(M, bits, eig, max_iter)
        return eig, bits, cents


class VaqMultiRefiner(_RefinerBase):
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
    _prefix = "vaqhip_multi_refiner_"
    _destroy = "vaqhip_multi_refiner_destroy"
    _check = staticmethod(_lib.check_multi)
    _Timing = _lib.MultiRefinerSearchTiming

    def __init__(self, devices: Sequence[int], D: int):
        self.D = int(D)
        self.devices = [int(d) for d in devices]
        self._exact = False
        self._h = C.c_void_p()
        h = C.c_void_p()
        devs = (C.c_int * len(self.devices))(*self.devices)
        _lib.check_multi(_lib.load().vaqhip_multi_refiner_create(C.byref(h), self.D, len(self.devices), devs))
        self._h = h

    def fit_quantiles(self, bits: Sequence[int], eigvec: Optional[np.ndarray] = None):
        """vaqhip_multi_refiner_lut_fit_quantiles: binaryEncodingLUT's quantile codebooks over the RAW rows resident on
        the shards, read in place (eigvec: D x D, applied first; None: the rows are their own image).  Returns
        (cent[D, 256], q[D, 257]), bit for bit the single fit's over all rows.  Byte rows (set_rows_u8) are read as
        they lie, a byte widened where it is loaded: the fit's result over the widened rows."""
        return _fit_quantiles_call(self.D, bits, eigvec, lambda L, b, e, c, q: L.vaqhip_multi_refiner_lut_fit_quantiles(
            self._h, b, e, c, q))

    def info(self) -> dict:
        """Shard rows, and the phase times of the last refine made under set_option("timing", 1) (waits for it)."""
        inf = _lib.MultiRefinerInfo()
        self._call("get_info", C.byref(inf))
        return _struct_dict(inf, cut=("device_ids", "shard_rows"))
