"""VaqHipFast: VaqHip with the FAST search method (uint8 tables over codes of at most 4 bits) and the forms of
VAQ::learnQuantization that fill its mOffsets / mScale."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._adapt import _dptr, _ptr, _same, _torch_stream, _u8_rows, _u8_rows_device, _wref
from .single import NNMethod, VaqHip


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
        self._learn_with(lambda off, sc: _lib.load().vaqhip_learn_quantization(
            self._h, _ptr(X), X.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

    def _learn_with(self, call) -> None:
        """The arrays around one of the five forms: call(off, sc) -> code; mOffsets / mScale on success."""
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
        _torch_stream(x.device).synchronize()
        self._learn_with(lambda off, sc: _lib.load().vaqhip_learn_quantization_device(
            self._h, _dptr(x), x.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

    def learnQuantization_u8_device(self, d_X, sampleRatio: float, projected: bool = False) -> None:
        """The same from a uint8 torch CUDA tensor (vaqhip_learn_quantization_u8_device); it may start at any byte."""
        x = _u8_rows_device(d_X, self.mTotalDim)
        self._ensure_index()
        _torch_stream(x.device).synchronize()
        self._learn_with(lambda off, sc: _lib.load().vaqhip_learn_quantization_u8_device(
            self._h, _dptr(x), x.shape[0], 1 if projected else 0, C.c_float(sampleRatio), off, sc))

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
