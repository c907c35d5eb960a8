"""ctypes binding of include/vaqhip.h (vaq_amd/lib/libvaqhip.so).

The library is loaded lazily and the load FAILS LOUDLY when the shared object
is missing: there is no Python/NumPy fallback for any entry point.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("VAQHIP_LIB") or os.path.join(_HERE, "lib", "libvaqhip.so")

# every symbol include/vaqhip.h declares
SYMBOLS = [
    "vaqhip_index_create", "vaqhip_index_create_ex", "vaqhip_index_destroy", "vaqhip_index_set_codes_u16",
    "vaqhip_index_set_codes_u16_device", "vaqhip_index_add_codes_u16", "vaqhip_index_add_codes_u16_device",
    "vaqhip_index_set_ti_clusters", "vaqhip_index_cluster_ti_kmeans", "vaqhip_last_kmeans_timing",
    "vaqhip_index_set_method",
    "vaqhip_index_set_lut_quantization", "vaqhip_learn_quantization", "vaqhip_build_small_lut",
    "vaqhip_search", "vaqhip_search_projected",
    "vaqhip_search_device", "vaqhip_search_staged_supported", "vaqhip_search_begin_device",
    "vaqhip_search_finish_device", "vaqhip_build_lut", "vaqhip_project", "vaqhip_merge_topk_device",
    "vaqhip_merge_topk_strided_device", "vaqhip_merge_fast_device",
    "vaqhip_encode", "vaqhip_encode_device",
    "vaqhip_lut_fit_quantiles", "vaqhip_lut_fit_quantiles_device", "vaqhip_lut_fit_set_timing",
    "vaqhip_last_lut_fit_timing", "vaqhip_index_set_lut_quantiles", "vaqhip_encode_lut", "vaqhip_encode_lut_device",
    "vaqhip_refine", "vaqhip_refine_device",
    "vaqhip_refiner_create", "vaqhip_refiner_destroy", "vaqhip_refiner_set_rows", "vaqhip_refiner_set_rows_device",
    "vaqhip_refiner_add_rows", "vaqhip_refiner_set_rows_u8", "vaqhip_refiner_set_rows_u8_device",
    "vaqhip_refiner_add_rows_u8", "vaqhip_refiner_elem_size", "vaqhip_refiner_set_option", "vaqhip_refiner_refine", "vaqhip_refiner_refine_device",
    "vaqhip_search_refine", "vaqhip_search_refine_device",
    "vaqhip_refiner_search", "vaqhip_refiner_search_device", "vaqhip_refiner_last_search_timing",
    "vaqhip_index_info", "vaqhip_set_option", "vaqhip_last_timing", "vaqhip_last_error",
    "vaqhip_version", "vaqhip_device_count",
    "vaqhip_multi_create", "vaqhip_multi_destroy", "vaqhip_multi_set_codes_u16", "vaqhip_multi_add_codes_u16",
    "vaqhip_multi_search", "vaqhip_multi_search_device", "vaqhip_multi_set_ti_clusters", "vaqhip_multi_set_method", "vaqhip_multi_set_option",
    "vaqhip_multi_set_lut_quantization", "vaqhip_multi_learn_quantization",
    "vaqhip_multi_cluster_ti_kmeans", "vaqhip_multi_last_kmeans_timing",
    "vaqhip_multi_get_info", "vaqhip_multi_shard", "vaqhip_multi_last_error",
    "vaqhip_multi_encode_set_codes", "vaqhip_multi_encode_add_codes", "vaqhip_multi_encode_from_refiner",
    "vaqhip_multi_last_encode_timing",
    "vaqhip_multi_set_lut_quantiles", "vaqhip_multi_encode_lut_set_codes", "vaqhip_multi_encode_lut_add_codes",
    "vaqhip_multi_encode_lut_from_refiner",
    "vaqhip_multi_lut_fit_quantiles", "vaqhip_multi_refiner_lut_fit_quantiles", "vaqhip_multi_last_lut_fit_timing",
    "vaqhip_multi_refiner_create", "vaqhip_multi_refiner_destroy", "vaqhip_multi_refiner_set_rows",
    "vaqhip_multi_refiner_add_rows", "vaqhip_multi_refiner_set_rows_u8", "vaqhip_multi_refiner_add_rows_u8",
    "vaqhip_multi_refiner_elem_size", "vaqhip_multi_refiner_set_option", "vaqhip_multi_refiner_refine",
    "vaqhip_multi_refiner_refine_device", "vaqhip_multi_search_refine", "vaqhip_multi_search_refine_device",
    "vaqhip_multi_refiner_get_info",
    "vaqhip_multi_refiner_search", "vaqhip_multi_refiner_search_device", "vaqhip_multi_refiner_last_search_timing",
    "vaqhip_encode_u8", "vaqhip_encode_u8_device", "vaqhip_encode_lut_u8", "vaqhip_encode_lut_u8_device",
    "vaqhip_lut_fit_quantiles_u8", "vaqhip_lut_fit_quantiles_u8_device",
    "vaqhip_multi_encode_set_codes_u8", "vaqhip_multi_encode_add_codes_u8",
    "vaqhip_multi_encode_lut_set_codes_u8", "vaqhip_multi_encode_lut_add_codes_u8",
    "vaqhip_multi_lut_fit_quantiles_u8",
    "vaqhip_learn_quantization_u8", "vaqhip_learn_quantization_device", "vaqhip_learn_quantization_u8_device",
    "vaqhip_learn_quantization_from_refiner", "vaqhip_learn_set_workspace", "vaqhip_last_learn_timing",
    "vaqhip_multi_learn_quantization_u8", "vaqhip_multi_learn_quantization_from_refiner",
    "vaqhip_fit_codebooks", "vaqhip_fit_codebooks_device", "vaqhip_fit_codebooks_u8", "vaqhip_fit_codebooks_u8_device",
    "vaqhip_refiner_fit_codebooks", "vaqhip_fit_codebooks_set_timing", "vaqhip_last_fit_codebooks_timing",
    "vaqhip_multi_fit_codebooks", "vaqhip_multi_fit_codebooks_u8", "vaqhip_multi_refiner_fit_codebooks",
    "vaqhip_multi_last_fit_codebooks_timing",
    "vaqhip_fit_codebooks_hier", "vaqhip_fit_codebooks_hier_device", "vaqhip_fit_codebooks_hier_u8",
    "vaqhip_fit_codebooks_hier_u8_device", "vaqhip_refiner_fit_codebooks_hier", "vaqhip_last_fit_codebooks_hier_timing",
    "vaqhip_fit_codebooks_bin", "vaqhip_fit_codebooks_bin_device", "vaqhip_fit_codebooks_bin_u8",
    "vaqhip_fit_codebooks_bin_u8_device", "vaqhip_refiner_fit_codebooks_bin", "vaqhip_last_fit_codebooks_bin_timing",
    "vaqhip_fit_codebooks_bin_set_sums",
    "vaqhip_train_moment", "vaqhip_train_moment_device", "vaqhip_train_moment_u8", "vaqhip_train_moment_u8_device",
    "vaqhip_refiner_train_moment", "vaqhip_sym_eigen_device", "vaqhip_sym_eigen_host", "vaqhip_train_plan",
    "vaqhip_allocate_bits", "vaqhip_train_rotation", "vaqhip_train_rotation_device", "vaqhip_train_rotation_u8",
    "vaqhip_train_rotation_u8_device", "vaqhip_refiner_train_rotation", "vaqhip_last_train_timing",
    "vaqhip_bitvec_create", "vaqhip_bitvec_destroy", "vaqhip_bitvec_set_rows", "vaqhip_bitvec_set_rows_device",
    "vaqhip_bitvec_add_rows", "vaqhip_bitvec_size", "vaqhip_bitvec_set_option", "vaqhip_bitvec_query",
    "vaqhip_bitvec_query_device", "vaqhip_bitvec_query_rerank", "vaqhip_bitvec_query_rerank_device",
]
MAX_DEVICES = 16

ERROR_NAMES = {
    -1: "EINVAL", -2: "EUNSUPPORTED", -3: "ENODEVICE", -4: "ENOMEM", -5: "EHIP",
    -6: "ERANGE", -7: "ESTATE", -8: "ENOCONV",
}


class VaqHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vaqhip error {code} ({ERROR_NAMES.get(code, '?')}): {msg}")
        self.code = code


class Info(C.Structure):
    _fields_ = [("D", C.c_int), ("M", C.c_int), ("L", C.c_int), ("max_bits", C.c_int),
                ("total_bits", C.c_int), ("code_bytes", C.c_int), ("algo_code_bytes", C.c_int),
                ("lut_floats", C.c_int), ("N", C.c_int64), ("id_base", C.c_int64),
                ("device_id", C.c_int), ("layout", C.c_int), ("ti_clusters", C.c_int),
                ("ti_segments", C.c_int), ("methods", C.c_uint), ("visit", C.c_float)]


class Timing(C.Structure):
    _fields_ = [("project_ms", C.c_float), ("lut_ms", C.c_float), ("seed_ms", C.c_float),
                ("scan_ms", C.c_float),
                ("merge_ms", C.c_float), ("n_searches", C.c_int), ("queries_per_pass", C.c_int), ("slices", C.c_int),
                ("workgroups", C.c_int), ("passes", C.c_int), ("lds_bytes", C.c_int),
                ("seed_slices", C.c_int), ("early_abandon", C.c_int),
                ("best_first", C.c_int), ("deferred_queries", C.c_int),
                ("bucket_major", C.c_int)]


class KmeansTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("assign_ms", C.c_float), ("accumulate_ms", C.c_float),
                ("update_ms", C.c_float), ("iterations", C.c_int), ("rows", C.c_int), ("dims", C.c_int),
                ("clusters", C.c_int)]


class LutFitTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("project_ms", C.c_float), ("extract_ms", C.c_float),
                ("sort_ms", C.c_float), ("quantile_ms", C.c_float), ("means_ms", C.c_float),
                ("rows", C.c_int64), ("dims", C.c_int)]


class FitCodebooksTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("gather_ms", C.c_float), ("assign_ms", C.c_float),
                ("accumulate_ms", C.c_float), ("update_ms", C.c_float), ("iterations", C.c_int),
                ("subspaces", C.c_int), ("dims", C.c_int), ("sample_rows", C.c_int64), ("rows", C.c_int64)]


class FitCodebooksHierTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("stage1_ms", C.c_float), ("regroup_ms", C.c_float), ("stage2_ms", C.c_float),
                ("groups", C.c_int), ("min_group_rows", C.c_int), ("max_group_rows", C.c_int),
                ("stage1_iterations", C.c_int), ("stage2_iterations", C.c_int), ("hier_subspaces", C.c_int),
                ("subspaces", C.c_int), ("dims", C.c_int), ("rows", C.c_int64)]


class FitCodebooksBinTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("fit_ms", C.c_float), ("split_ms", C.c_float), ("cut_ms", C.c_float),
                ("levels", C.c_int), ("nodes", C.c_int), ("cut_nodes", C.c_int), ("resampled_fits", C.c_int),
                ("leaf_nodes", C.c_int), ("min_leaf_rows", C.c_int), ("max_leaf_rows", C.c_int),
                ("max_iterations", C.c_int), ("bin_subspaces", C.c_int), ("subspaces", C.c_int), ("dims", C.c_int),
                ("rows", C.c_int64)]


class TrainTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("moment_ms", C.c_float), ("eigen_ms", C.c_float), ("finish_ms", C.c_float),
                ("plan_ms", C.c_float),
                ("sweeps", C.c_int), ("subspaces", C.c_int), ("dims", C.c_int), ("sample_rows", C.c_int64),
                ("rows", C.c_int64)]


class LearnTiming(C.Structure):
    _fields_ = [("sample_rows", C.c_int), ("column_groups", C.c_int), ("chosen_alpha", C.c_int),
                ("gather_ms", C.c_float), ("tables_ms", C.c_float), ("sort_ms", C.c_float),
                ("order_stats_ms", C.c_float), ("loss_ms", C.c_float), ("total_ms", C.c_float),
                ("loss", C.c_double * 7)]


class RefinerSearchTiming(C.Structure):
    _fields_ = [("select_ms", C.c_float), ("merge_ms", C.c_float), ("flag_ms", C.c_float), ("replay_ms", C.c_float),
                ("listed_queries", C.c_int), ("splits", C.c_int), ("workgroups", C.c_int),
                ("queries_per_group", C.c_int), ("register_form", C.c_int)]


class MultiRefinerSearchTiming(C.Structure):
    _fields_ = RefinerSearchTiming._fields_ + [("gather_ms", C.c_float), ("cross_merge_ms", C.c_float),
                                               ("chain_ms", C.c_float), ("chain_shards", C.c_int), ("sets", C.c_int)]


class MultiEncodeTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("encode_ms", C.c_float), ("set_codes_ms", C.c_float), ("rows", C.c_int64),
                ("n_devices", C.c_int)]


class MultiLutFitTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("columns_ms", C.c_float), ("copy_ms", C.c_float), ("sort_ms", C.c_float),
                ("quantile_ms", C.c_float), ("means_ms", C.c_float), ("rows", C.c_int64), ("dims", C.c_int),
                ("n_devices", C.c_int)]


class MultiFitCodebooksTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("columns_ms", C.c_float), ("copy_ms", C.c_float), ("place_ms", C.c_float),
                ("assign_ms", C.c_float), ("accumulate_ms", C.c_float), ("update_ms", C.c_float),
                ("iterations", C.c_int), ("subspaces", C.c_int), ("dims", C.c_int), ("rows", C.c_int64),
                ("sample_rows", C.c_int64), ("n_devices", C.c_int), ("owner_subspaces", C.c_int * 16)]


class MultiInfo(C.Structure):
    _fields_ = [("n_devices", C.c_int), ("exchange", C.c_int), ("N", C.c_int64), ("id_base", C.c_int64),
                ("device_ids", C.c_int * 16), ("shard_rows", C.c_int64 * 16), ("last_search_ms", C.c_float),
                ("last_exchange_ms", C.c_float), ("last_merge_ms", C.c_float)]


class MultiRefinerInfo(C.Structure):
    _fields_ = [("n_devices", C.c_int), ("D", C.c_int), ("N", C.c_int64), ("id_base", C.c_int64),
                ("device_ids", C.c_int * 16), ("shard_rows", C.c_int64 * 16), ("exact_ties", C.c_int),
                ("set_queries", C.c_int), ("last_sets", C.c_int), ("last_broadcast_ms", C.c_float),
                ("last_distances_ms", C.c_float), ("last_gather_ms", C.c_float), ("last_select_ms", C.c_float)]


_lib = None


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Return the loaded C-ABI library; raise if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} is missing: build it with `python -m vaq_amd.build` "
            "(hipcc, gfx950). vaq_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 /
    # libhsa-runtime64 under torch/lib, and a second copy (the system one this
    # library's RUNPATH points at) cannot open the GPU once the first has.  Both
    # carry the soname libamdhip64.so.7, so importing torch first makes the
    # dynamic linker bind libvaqhip.so to the runtime torch already loaded.
    # Without torch (a plain C/C++ host) the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.vaqhip_index_create.argtypes = [C.POINTER(vp), i32, i32, C.POINTER(i32),
                                      C.POINTER(C.POINTER(C.c_float)), vp, i32]
    L.vaqhip_index_create_ex.argtypes = [C.POINTER(vp), i32, i32, C.POINTER(i32),
                                         C.POINTER(C.POINTER(C.c_float)), vp, i32, C.c_uint]
    L.vaqhip_index_destroy.argtypes = [vp]
    L.vaqhip_index_destroy.restype = None
    L.vaqhip_index_set_codes_u16.argtypes = [vp, vp, i64, i64]
    L.vaqhip_index_set_codes_u16_device.argtypes = [vp, vp, i64, i64, vp]
    L.vaqhip_index_add_codes_u16.argtypes = [vp, vp, i64]
    L.vaqhip_index_add_codes_u16_device.argtypes = [vp, vp, i64, vp]
    L.vaqhip_index_set_ti_clusters.argtypes = [vp, vp, i32, i32]
    L.vaqhip_index_cluster_ti_kmeans.argtypes = [vp, i32, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.vaqhip_last_kmeans_timing.argtypes = [vp, C.POINTER(KmeansTiming)]
    L.vaqhip_index_set_method.argtypes = [vp, C.c_uint, C.c_float]
    L.vaqhip_index_set_lut_quantization.argtypes = [vp, vp, vp]
    L.vaqhip_learn_quantization.argtypes = [vp, vp, i64, i32, C.c_float, vp, vp]
    L.vaqhip_build_small_lut.argtypes = [vp, vp, i32, i32, vp]
    for name in ("vaqhip_learn_quantization_u8", "vaqhip_learn_quantization_device",
                 "vaqhip_learn_quantization_u8_device", "vaqhip_multi_learn_quantization_u8"):
        getattr(L, name).argtypes = [vp, vp, i64, i32, C.c_float, vp, vp]
    L.vaqhip_learn_quantization_from_refiner.argtypes = [vp, vp, C.c_float, vp, vp]
    L.vaqhip_multi_learn_quantization_from_refiner.argtypes = [vp, vp, C.c_float, vp, vp]
    L.vaqhip_learn_set_workspace.argtypes = [i64]
    L.vaqhip_last_learn_timing.argtypes = [vp, C.POINTER(LearnTiming)]
    L.vaqhip_search.argtypes = [vp, vp, i32, i32, vp, vp]
    L.vaqhip_search_projected.argtypes = [vp, vp, i32, i32, vp, vp]
    L.vaqhip_search_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.vaqhip_search_staged_supported.argtypes = [vp, i32, i32]
    L.vaqhip_search_begin_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.vaqhip_search_finish_device.argtypes = [vp, vp, vp]
    L.vaqhip_build_lut.argtypes = [vp, vp, i32, i32, vp]
    L.vaqhip_project.argtypes = [vp, vp, i64, vp]
    L.vaqhip_merge_topk_device.argtypes = [i32, vp, vp, i32, i32, i32, vp, vp, vp]
    L.vaqhip_encode.argtypes = [vp, vp, i64, i32, vp]
    L.vaqhip_encode_device.argtypes = [vp, vp, i64, i32, vp, vp]
    L.vaqhip_lut_fit_quantiles.argtypes = [i32, vp, i64, i32, C.POINTER(i32), vp, vp, vp]
    L.vaqhip_lut_fit_quantiles_device.argtypes = [i32, vp, i64, i32, C.POINTER(i32), vp, vp, vp, vp]
    L.vaqhip_lut_fit_set_timing.argtypes = [i32]
    L.vaqhip_last_lut_fit_timing.argtypes = [C.POINTER(LutFitTiming)]
    L.vaqhip_index_set_lut_quantiles.argtypes = [vp, vp]
    for name in ("vaqhip_fit_codebooks", "vaqhip_fit_codebooks_u8", "vaqhip_fit_codebooks_hier", "vaqhip_fit_codebooks_hier_u8",
                 "vaqhip_fit_codebooks_bin", "vaqhip_fit_codebooks_bin_u8"):
        getattr(L, name).argtypes = [i32, vp, i64, i32, i32, C.POINTER(i32), vp, i32, vp, vp, vp]
    for name in ("vaqhip_fit_codebooks_device", "vaqhip_fit_codebooks_u8_device", "vaqhip_fit_codebooks_hier_device",
                 "vaqhip_fit_codebooks_hier_u8_device", "vaqhip_fit_codebooks_bin_device", "vaqhip_fit_codebooks_bin_u8_device"):
        getattr(L, name).argtypes = [i32, vp, i64, i32, i32, C.POINTER(i32), vp, i32, vp, vp, vp, vp]
    L.vaqhip_refiner_fit_codebooks.argtypes = [vp, i32, C.POINTER(i32), vp, i32, vp, vp, vp]
    L.vaqhip_refiner_fit_codebooks_hier.argtypes = [vp, i32, C.POINTER(i32), vp, i32, vp, vp, vp]
    L.vaqhip_last_fit_codebooks_hier_timing.argtypes = [C.POINTER(FitCodebooksHierTiming)]
    L.vaqhip_refiner_fit_codebooks_bin.argtypes = [vp, i32, C.POINTER(i32), vp, i32, vp, vp, vp]
    L.vaqhip_last_fit_codebooks_bin_timing.argtypes = [C.POINTER(FitCodebooksBinTiming)]
    L.vaqhip_fit_codebooks_bin_set_sums.argtypes = [i32]
    L.vaqhip_fit_codebooks_set_timing.argtypes = [i32]
    L.vaqhip_last_fit_codebooks_timing.argtypes = [C.POINTER(FitCodebooksTiming)]
    for name in ("vaqhip_train_moment", "vaqhip_train_moment_u8"):
        getattr(L, name).argtypes = [i32, vp, i64, i32, vp, vp]
    for name in ("vaqhip_train_moment_device", "vaqhip_train_moment_u8_device"):
        getattr(L, name).argtypes = [i32, vp, i64, i32, vp, vp, vp]
    L.vaqhip_refiner_train_moment.argtypes = [vp, vp, vp]
    L.vaqhip_sym_eigen_device.argtypes = [i32, vp, i32, vp, vp, C.POINTER(i32), vp]
    L.vaqhip_sym_eigen_host.argtypes = [vp, i32, vp, vp, C.POINTER(i32)]
    L.vaqhip_train_plan.argtypes = [vp, i32, i32, C.c_float, i32, i32, vp, vp, vp, vp, C.POINTER(i32), vp, vp,
                                    C.POINTER(i32)]
    L.vaqhip_allocate_bits.argtypes = [vp, i32, vp, i32, vp, i32, vp, C.POINTER(C.c_double)]
    for name in ("vaqhip_train_rotation", "vaqhip_train_rotation_u8"):
        getattr(L, name).argtypes = [i32, vp, i64, i32, i32, i32, i32, i32, C.c_float, vp, vp, vp, C.POINTER(i32)]
    for name in ("vaqhip_train_rotation_device", "vaqhip_train_rotation_u8_device"):
        getattr(L, name).argtypes = [i32, vp, i64, i32, i32, i32, i32, i32, C.c_float, vp, vp, vp, C.POINTER(i32), vp]
    L.vaqhip_refiner_train_rotation.argtypes = [vp, i32, i32, i32, i32, C.c_float, vp, vp, vp, C.POINTER(i32)]
    L.vaqhip_last_train_timing.argtypes = [C.POINTER(TrainTiming)]
    L.vaqhip_encode_lut.argtypes = [vp, vp, i64, i32, vp]
    L.vaqhip_encode_lut_device.argtypes = [vp, vp, i64, i32, vp, vp]
    L.vaqhip_refine.argtypes = [i32, vp, i32, i32, vp, i64, vp, i32, i32, vp, vp]
    L.vaqhip_refine_device.argtypes = [i32, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp]
    L.vaqhip_refiner_create.argtypes = [C.POINTER(vp), i32, i32]
    L.vaqhip_refiner_destroy.argtypes = [vp]
    L.vaqhip_refiner_destroy.restype = None
    L.vaqhip_refiner_set_rows.argtypes = [vp, vp, i64, i64]
    L.vaqhip_refiner_set_rows_device.argtypes = [vp, vp, i64, i64, vp]
    L.vaqhip_refiner_add_rows.argtypes = [vp, vp, i64]
    L.vaqhip_refiner_set_rows_u8.argtypes = [vp, vp, i64, i64]
    L.vaqhip_refiner_set_rows_u8_device.argtypes = [vp, vp, i64, i64, vp]
    L.vaqhip_refiner_add_rows_u8.argtypes = [vp, vp, i64]
    L.vaqhip_refiner_elem_size.argtypes = [vp]
    L.vaqhip_refiner_set_option.argtypes = [vp, C.c_char_p, i64]
    L.vaqhip_refiner_refine.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp]
    L.vaqhip_refiner_refine_device.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp]
    L.vaqhip_refiner_search.argtypes = [vp, vp, i32, i32, vp, vp]
    L.vaqhip_refiner_search_device.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.vaqhip_refiner_last_search_timing.argtypes = [vp, C.POINTER(RefinerSearchTiming)]
    L.vaqhip_search_refine.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.vaqhip_search_refine_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.vaqhip_merge_topk_strided_device.argtypes = [i32, vp, vp, i32, i64, i64, i32, i32, vp, vp, vp]
    L.vaqhip_merge_fast_device.argtypes = [i32, vp, i64, i32, i64, vp, vp, i32, i64, i64, i32, i32, vp, vp, vp]
    L.vaqhip_bitvec_create.argtypes = [C.POINTER(vp), i32, i32]
    L.vaqhip_bitvec_destroy.argtypes = [vp]
    L.vaqhip_bitvec_destroy.restype = None
    L.vaqhip_bitvec_set_rows.argtypes = [vp, vp, i64, i64]
    L.vaqhip_bitvec_set_rows_device.argtypes = [vp, vp, i64, i64, vp]
    L.vaqhip_bitvec_add_rows.argtypes = [vp, vp, i64]
    L.vaqhip_bitvec_size.argtypes = [vp]
    L.vaqhip_bitvec_size.restype = i64
    L.vaqhip_bitvec_set_option.argtypes = [vp, C.c_char_p, i64]
    L.vaqhip_bitvec_query.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.vaqhip_bitvec_query_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.vaqhip_bitvec_query_rerank.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.vaqhip_bitvec_query_rerank_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.vaqhip_index_info.argtypes = [vp, C.POINTER(Info)]
    L.vaqhip_set_option.argtypes = [vp, C.c_char_p, i64]
    L.vaqhip_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.vaqhip_last_error.restype = C.c_char_p
    L.vaqhip_multi_create.argtypes = [C.POINTER(vp), i32, i32, C.POINTER(i32), C.POINTER(C.POINTER(C.c_float)), vp,
                                      i32, C.POINTER(i32), C.c_uint]
    L.vaqhip_multi_destroy.argtypes = [vp]
    L.vaqhip_multi_destroy.restype = None
    L.vaqhip_multi_set_codes_u16.argtypes = [vp, vp, i64, i64]
    L.vaqhip_multi_add_codes_u16.argtypes = [vp, vp, i64]
    L.vaqhip_multi_search.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.vaqhip_multi_search_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.vaqhip_multi_set_ti_clusters.argtypes = [vp, vp, i32, i32]
    L.vaqhip_multi_set_method.argtypes = [vp, C.c_uint, C.c_float]
    L.vaqhip_multi_set_option.argtypes = [vp, C.c_char_p, i64]
    L.vaqhip_multi_set_lut_quantization.argtypes = [vp, vp, vp]
    L.vaqhip_multi_learn_quantization.argtypes = [vp, vp, i64, i32, C.c_float, vp, vp]
    L.vaqhip_multi_cluster_ti_kmeans.argtypes = [vp, i32, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.vaqhip_multi_last_kmeans_timing.argtypes = [vp, C.POINTER(KmeansTiming)]
    L.vaqhip_multi_get_info.argtypes = [vp, C.POINTER(MultiInfo)]
    L.vaqhip_multi_shard.argtypes = [vp, i32]
    L.vaqhip_multi_shard.restype = vp
    L.vaqhip_multi_last_error.restype = C.c_char_p
    L.vaqhip_multi_encode_set_codes.argtypes = [vp, vp, i64, i32, i64, vp]
    L.vaqhip_multi_encode_add_codes.argtypes = [vp, vp, i64, i32, vp]
    L.vaqhip_multi_encode_from_refiner.argtypes = [vp, vp, vp]
    L.vaqhip_multi_last_encode_timing.argtypes = [vp, C.POINTER(MultiEncodeTiming)]
    L.vaqhip_multi_set_lut_quantiles.argtypes = [vp, vp]
    L.vaqhip_multi_encode_lut_set_codes.argtypes = [vp, vp, i64, i32, i64, vp]
    L.vaqhip_multi_encode_lut_add_codes.argtypes = [vp, vp, i64, i32, vp]
    L.vaqhip_multi_encode_lut_from_refiner.argtypes = [vp, vp, vp]
    L.vaqhip_multi_lut_fit_quantiles.argtypes = [i32, C.POINTER(i32), vp, i64, i32, C.POINTER(i32), vp, vp, vp]
    L.vaqhip_multi_refiner_lut_fit_quantiles.argtypes = [vp, C.POINTER(i32), vp, vp, vp]
    L.vaqhip_multi_last_lut_fit_timing.argtypes = [C.POINTER(MultiLutFitTiming)]
    for name in ("vaqhip_multi_fit_codebooks", "vaqhip_multi_fit_codebooks_u8"):
        getattr(L, name).argtypes = [i32, C.POINTER(i32), vp, i64, i32, i32, C.POINTER(i32), vp, i32, vp, vp, vp]
    L.vaqhip_multi_refiner_fit_codebooks.argtypes = [vp, i32, C.POINTER(i32), vp, i32, vp, vp, vp]
    L.vaqhip_multi_last_fit_codebooks_timing.argtypes = [C.POINTER(MultiFitCodebooksTiming)]
    L.vaqhip_multi_refiner_create.argtypes = [C.POINTER(vp), i32, i32, C.POINTER(i32)]
    L.vaqhip_multi_refiner_destroy.argtypes = [vp]
    L.vaqhip_multi_refiner_destroy.restype = None
    L.vaqhip_multi_refiner_set_rows.argtypes = [vp, vp, i64, i64]
    L.vaqhip_multi_refiner_add_rows.argtypes = [vp, vp, i64]
    L.vaqhip_multi_refiner_set_rows_u8.argtypes = [vp, vp, i64, i64]
    L.vaqhip_multi_refiner_add_rows_u8.argtypes = [vp, vp, i64]
    L.vaqhip_multi_refiner_elem_size.argtypes = [vp]
    L.vaqhip_multi_refiner_set_option.argtypes = [vp, C.c_char_p, i64]
    L.vaqhip_multi_refiner_refine.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp]
    L.vaqhip_multi_refiner_refine_device.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp]
    L.vaqhip_multi_search_refine.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.vaqhip_multi_search_refine_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.vaqhip_multi_refiner_get_info.argtypes = [vp, C.POINTER(MultiRefinerInfo)]
    L.vaqhip_multi_refiner_search.argtypes = [vp, vp, i32, i32, vp, vp]
    L.vaqhip_multi_refiner_search_device.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.vaqhip_multi_refiner_last_search_timing.argtypes = [vp, C.POINTER(MultiRefinerSearchTiming)]
    for name in ("vaqhip_encode", "vaqhip_encode_device", "vaqhip_encode_lut", "vaqhip_encode_lut_device",
                 "vaqhip_lut_fit_quantiles", "vaqhip_lut_fit_quantiles_device", "vaqhip_multi_encode_set_codes",
                 "vaqhip_multi_encode_add_codes", "vaqhip_multi_encode_lut_set_codes",
                 "vaqhip_multi_encode_lut_add_codes", "vaqhip_multi_lut_fit_quantiles"):
        # the byte-row twins: the float call's argument list, the rows a void pointer either way
        u8 = name[:-len("_device")] + "_u8_device" if name.endswith("_device") else name + "_u8"
        getattr(L, u8).argtypes = getattr(L, name).argtypes
    for name in SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int:
            fn.restype = C.c_int
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        msg = load().vaqhip_last_error()
        raise VaqHipError(rc, msg.decode() if msg else "")
    return rc


def check_multi(rc: int) -> int:
    if rc < 0:
        msg = load().vaqhip_multi_last_error()
        raise VaqHipError(rc, msg.decode() if msg else "")
    return rc
