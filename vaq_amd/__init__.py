"""vaq_amd -- MI355X (gfx950) implementation of VAQ's quantized-distance search path.

Product surface:
  include/vaqhip.h            C ABI (the drop-in boundary)
  include/vaqhip.hpp          C++ adapter with the reference's names (class VaqHip)
  vaq_amd.VaqHip              Python mirror of the same interface, over the C ABI
  vaq_amd.VaqHipFast          the same with the FAST search method (uint8 tables, 4-bit codes)
  vaq_amd.VaqRefiner          VAQ::refine over raw rows resident on the device, reference-exact
  vaq_amd.VaqMultiRefiner     the same over raw rows sharded across several GPUs
  vaq_amd.VaqBitVec           BitVecEngine::query / ::queryRerank (QueryMethod::Sort) over packed bit rows on the device
  vaq_amd.lut_fit_quantiles_multi  binaryEncodingLUT's quantile codebooks with the rows cut over several GPUs
  vaq_amd.lut_fit_quantiles_multi_u8  the same from byte rows (a bvecs dataset as its file holds it)
  vaq_amd.fit_codebooks       the subspace codebooks (KMeans::staticFitSampling per subspace) from raw rows
  vaq_amd.fit_codebooks_u8    the same from byte rows; VaqRefiner.fit_codebooks over resident rows
  fit_codebooks(devices=[...])  the same fit with the rows cut over several GPUs, one owner per subspace, bit for bit;
                              VaqMultiRefiner.fit_codebooks over sharded resident rows; last_multi_fit_codebooks_timing
  vaq_amd.train_rotation      VAQ::train's front half from raw rows: second-moment PCA and variance-aware bits
  vaq_amd.fit_codebooks_hier  the hierarchical form (--kmeans-ver 1): subspaces above 8 bits as 128 x 2^(bits-7) centres;
                              fit_codebooks_hier_u8, VaqRefiner.fit_codebooks_hier, last_fit_codebooks_hier_timing
  vaq_amd.fit_codebooks_bin   the binary-tree form (--kmeans-ver 2's rule): subspaces above 8 bits as a tree of 2-centre fits,
                              no group size refused; fit_codebooks_bin_u8, VaqRefiner.fit_codebooks_bin,
                              last_fit_codebooks_bin_timing
  vaq_amd.train               the same chained into fit_codebooks; VaqRefiner.train_rotation / .train over resident rows
There is no CPU path: importing works anywhere, but every compute call needs
the HIP library and a GPU and raises otherwise.
"""
from ._lib import VaqHipError, lib_path, load  # noqa: F401
from .index import LabelDistVec, NNMethod, VaqHip, VaqHipFast, VaqHipMulti, VaqMultiRefiner, VaqRefiner  # noqa: F401
from .index import last_lut_fit_multi_timing, lut_fit_quantiles_multi, lut_fit_quantiles_multi_u8  # noqa: F401
from .index import fit_codebooks, fit_codebooks_timing, fit_codebooks_u8, last_fit_codebooks_timing  # noqa: F401
from .index import last_multi_fit_codebooks_timing  # noqa: F401
from .index import fit_codebooks_hier, fit_codebooks_hier_u8, last_fit_codebooks_hier_timing  # noqa: F401
from .index import fit_codebooks_bin, fit_codebooks_bin_u8, last_fit_codebooks_bin_timing  # noqa: F401
from .index import last_train_timing, train, train_rotation  # noqa: F401
from .index import QueryMethod, VaqBitVec  # noqa: F401

__all__ = ["VaqHip", "VaqHipFast", "VaqHipMulti", "VaqRefiner", "VaqMultiRefiner", "NNMethod", "LabelDistVec", "VaqHipError", "load", "lib_path",
           "lut_fit_quantiles_multi", "lut_fit_quantiles_multi_u8", "last_lut_fit_multi_timing",
           "fit_codebooks", "fit_codebooks_u8", "fit_codebooks_timing", "last_fit_codebooks_timing",
           "last_multi_fit_codebooks_timing", "fit_codebooks_hier", "fit_codebooks_hier_u8",
           "last_fit_codebooks_hier_timing", "fit_codebooks_bin", "fit_codebooks_bin_u8", "last_fit_codebooks_bin_timing",
           "train_rotation", "train", "last_train_timing", "VaqBitVec", "QueryMethod"]
