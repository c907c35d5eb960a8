"""Python mirror of the reference's `class VAQ` search interface (bitvecengine/VAQ.hpp:36-113) over the C ABI of
include/vaqhip.h.  This module only gathers the names; the code is one module per concern:

  single.py   NNMethod, LabelDistVec, VaqHip          fast.py    VaqHipFast
  refiner.py  VaqRefiner, VaqMultiRefiner             multi.py   VaqHipMulti
  fits.py     fit_codebooks*, lut_fit_quantiles_multi*, train_rotation, train, their timing calls
  merge.py    merge_topk_device, merge_topk_packed_device, merge_fast_device
  bitvec.py   VaqBitVec, QueryMethod (the Hamming queries of BitVecEngine)
  _adapt.py   what they share (pointers, row checks, the output pair and stream of a device call, handle lifetime)

All compute goes through libvaqhip.so; nothing here has a NumPy fallback.
"""
from . import _lib  # noqa: F401
from ._adapt import _ptr, _same, _u8_rows, _u8_rows_device, _wref  # noqa: F401
from .bitvec import QueryMethod, VaqBitVec  # noqa: F401
from .fast import VaqHipFast  # noqa: F401
from .fits import fit_codebooks_hier, fit_codebooks_hier_u8, last_fit_codebooks_hier_timing  # noqa: F401
from .fits import fit_codebooks_bin, fit_codebooks_bin_u8, last_fit_codebooks_bin_timing, fit_codebooks_bin_sums  # noqa: F401
from .fits import (_fit_codebooks_call, _fit_quantiles_call, fit_codebooks, fit_codebooks_timing,  # noqa: F401
                   fit_codebooks_u8, last_fit_codebooks_timing, last_lut_fit_multi_timing,
                   last_multi_fit_codebooks_timing, last_train_timing, lut_fit_quantiles_multi,
                   lut_fit_quantiles_multi_u8, train, train_rotation)
from .merge import merge_fast_device, merge_topk_device, merge_topk_packed_device  # noqa: F401
from .multi import VaqHipMulti  # noqa: F401
from .refiner import VaqMultiRefiner, VaqRefiner  # noqa: F401
from .single import LabelDistVec, NNMethod, VaqHip  # noqa: F401
