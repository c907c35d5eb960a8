"""tests/bitvec_ref.py (the restatement the GPU tests of the Hamming engine check against) against the fixtures of
tests/golden/hamming, which the compiled reference's KNNFromDists recorded -- and against that function live where
oracle/_ref is built.  Also what of the new surface needs no GPU: harness.sign_bits, the symbols, the refusals a
null handle or an oversized row gets before a device is looked for."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import bitvec_ref as br
from oracle import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "hamming")


def fixtures(prefix):
    files = sorted(glob.glob(os.path.join(GOLD, prefix + "*.npz")))
    assert files
    return [pytest.param(f, id=os.path.basename(f)[:-4]) for f in files]


@pytest.mark.parametrize("path", fixtures("hamming_"))
def test_query_sort_matches_fixture(path):
    g = np.load(path)
    lab, dis = br.query_sort(g["rows"], g["queries"], int(g["k"]))
    assert np.array_equal(lab, g["labels"])
    assert np.array_equal(dis, g["dists"])


@pytest.mark.parametrize("path", fixtures("rerank_"))
def test_query_rerank_matches_fixture(path):
    g = np.load(path)
    k, factor = int(g["k"]), int(g["factor"])
    cand, _ = br.query_sort(g["rows"], g["queries"], min(factor * k, g["rows"].shape[0]))
    assert np.array_equal(cand, g["candidates"])
    lab, dis = br.query_rerank(g["rows"], g["queries"], g["X"], g["XQ"], k, factor)
    assert np.array_equal(lab, g["labels"])
    assert np.array_equal(dis, g["dists"])


def test_fixtures_are_not_vacuous():
    """what make_hamming_golden.py asserts when it records, checked again on what is committed"""
    big_head = False
    for p in glob.glob(os.path.join(GOLD, "hamming_*.npz")):
        g = np.load(p)
        k = int(g["k"])
        d = br.hamming_dists(g["rows"], g["queries"])
        s = np.sort(d, axis=1)
        assert (s[:, k - 1] == s[:, k]).any(), p
        big_head |= k > 16 and any(len(np.unique(d[q, :k])) < k for q in range(d.shape[0]))
    assert big_head
    for p in glob.glob(os.path.join(GOLD, "rerank_*.npz")):
        g = np.load(p)
        k = int(g["k"])
        inside = across = False
        for q in range(g["queries"].shape[0]):
            e = br.euclidean_no_sqrt(g["XQ"][q], g["X"][g["candidates"][q]])
            assert e.max() <= 32767
            inside |= len(np.unique(e[:k])) < k
            s = np.sort(e)
            across |= bool(s[k - 1] == s[k])
        assert inside and across, p


def test_indices_supplied_is_dist_seq_order():
    """KNNFromDistsIndicesSupplied written out (sort, then insertions) is the k smallest by (dist, position), the
    head's position being std::sort's: the form the device kernel computes"""
    rs = np.random.RandomState(5)
    for n, k, top in ((40, 7, 4), (300, 40, 6), (1024, 100, 9), (64, 64, 3), (33, 32, 2)):
        d = rs.randint(0, top, n).astype(np.float32)
        idx = rs.permutation(n).astype(np.int32)
        got_i, got_d = br.knn_from_dists_indices_supplied(d, idx, k)
        head = br.std_sort_perm_f32(d[:k])
        order = np.concatenate([head, np.arange(k, n)])
        keys = d[order]
        best = np.argsort(keys, kind="stable")[:k]
        assert np.array_equal(got_i, idx[order][best])
        assert np.array_equal(got_d, keys[best])


@pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref is not built")
def test_against_compiled_reference():
    rs = np.random.RandomState(9)
    for n, k, top in ((50, 50, 3), (200, 17, 5), (900, 100, 12), (1500, 1024, 30)):
        d = rs.randint(0, top, n)
        idx, dist = po.ref_knn_from_dists(d.astype(np.int16), k)
        # KNNFromDists through query_sort's path
        import fast_ref
        lab, _ = fast_ref.knn_from_dists(d, k)
        assert np.array_equal(lab, idx)
        # KNNFromDistsIndicesSupplied over the same numbers as floats: idx = indices[knn.idx]
        perm = rs.permutation(n).astype(np.int32)
        gi, gd = br.knn_from_dists_indices_supplied(d.astype(np.float32), perm, k)
        assert np.array_equal(gi, perm[idx])
        assert np.array_equal(gd, dist.astype(np.float32))


def test_sign_bits():
    from vaq_amd import harness
    X = np.zeros((3, 70), np.float32)
    X[0, 0] = 1
    X[0, 63] = 2
    X[1, 64] = 1
    X[1, 69] = 1
    X[2] = -1
    b = harness.sign_bits(X)
    assert b.dtype == np.uint64 and b.shape == (3, 2)
    assert b.tolist() == [[0x8000000000000001, 0], [0, 0x8400000000000000], [0, 0]]
    assert np.array_equal(br.hamming_dists(b, b[:1])[0], [0, 4, 2])


def test_symbols_and_host_side_refusals(vaqlib):
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 122
    for s in ("create", "destroy", "set_rows", "set_rows_device", "add_rows", "size", "set_option", "query", "query_device",
              "query_rerank", "query_rerank_device"):
        assert hasattr(vaqlib, "vaqhip_bitvec_" + s) and "vaqhip_bitvec_" + s in _lib.SYMBOLS
    h = C.c_void_p()
    assert vaqlib.vaqhip_bitvec_create(C.byref(h), 0, 0) == -1
    assert vaqlib.vaqhip_bitvec_create(C.byref(h), 0, 1025) == -2 and b"16" in vaqlib.vaqhip_last_error()
    assert vaqlib.vaqhip_bitvec_create(None, 0, 64) == -1
    assert vaqlib.vaqhip_bitvec_query(None, None, 1, 1, 1, None, None) == -1
    assert vaqlib.vaqhip_bitvec_query_rerank(None, None, None, None, 1, 1, 1, None, None) == -1
    assert vaqlib.vaqhip_bitvec_set_option(None, b"dist_chunk_bytes", 1) == -1
    assert vaqlib.vaqhip_bitvec_size(None) == -1
    import vaq_amd
    assert vaq_amd.QueryMethod.Sort == 1 and vaq_amd.QueryMethod.SortEarlyAbandon == 3
