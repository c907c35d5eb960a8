"""The refusals of vaqhip_bitvec_query_naive_ti and vaqhip_bitvec_set_ti_clusters_from_refiner that are made before a
handle is looked into, with their codes; no device.  (nq == 0 and the query before the build need an engine, which needs
a device: tests/test_bitvec_ti_gpu.py::test_state.)"""
import ctypes as C

import pytest

from vaq_amd import _lib

P = C.c_void_p(64)  # never dereferenced on these paths


@pytest.mark.parametrize("case,code", [("null_engine", -1), ("null_refiner", -1), ("method_sort", -2),
                                       ("method_heap_early_abandon", -2), ("method_sort_early_abandon", -2), ("method_4", -1),
                                       ("method_minus_1", -1), ("k_0", -1), ("k_1025", -2), ("nq_negative", -1),
                                       ("null_queries", -1), ("null_labels", -1), ("null_distances", -1)])
@pytest.mark.parametrize("device_form", [False, True])
def test_query_refusals(vaqlib, case, code, device_form):
    a = dict(bv=P, r=P, q=P, nq=2, k=3, method=0, lab=P, dis=P)
    a.update({"null_engine": dict(bv=None), "null_refiner": dict(r=None), "method_sort": dict(method=1),
              "method_heap_early_abandon": dict(method=2), "method_sort_early_abandon": dict(method=3),
              "method_4": dict(method=4), "method_minus_1": dict(method=-1), "k_0": dict(k=0), "k_1025": dict(k=1025),
              "nq_negative": dict(nq=-1), "null_queries": dict(q=None), "null_labels": dict(lab=None),
              "null_distances": dict(dis=None)}[case])
    args = [a["bv"], a["r"], a["q"], a["nq"], a["k"], a["method"], a["lab"], a["dis"], None]
    fn = vaqlib.vaqhip_bitvec_query_naive_ti_device if device_form else vaqlib.vaqhip_bitvec_query_naive_ti
    assert fn(*(args + [None] if device_form else args)) == code
    assert vaqlib.vaqhip_last_error()


@pytest.mark.parametrize("bv,r,cen,T,D", [(None, P, P, 4, 8), (P, None, P, 4, 8), (P, P, None, 4, 8), (P, P, P, 0, 8),
                                          (P, P, P, 4097, 8), (P, P, P, 4, 0), (P, P, P, 4, 8177)])
def test_build_refusals(vaqlib, bv, r, cen, T, D):
    assert vaqlib.vaqhip_bitvec_set_ti_clusters_from_refiner(bv, r, cen, T, D) == -1
    assert "vaqhip_bitvec_set_ti_clusters_from_refiner" in _lib.SYMBOLS
