"""tests/bitvec_ref.py (the restatement the GPU tests of the Hamming engine check against) against the fixtures of
tests/golden/hamming, which the compiled reference's KNNFromDists recorded -- and against that function live where
oracle/_ref is built.  Also what of the new surface needs no GPU: harness.sign_bits, the symbols, the refusals a
null handle or an oversized row gets before a device is looked for."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import bitvec_cases as bc
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
    big_head, far = False, 0
    for p in glob.glob(os.path.join(GOLD, "hamming_*.npz")):
        g = np.load(p)
        k = int(g["k"])
        d = br.hamming_dists(g["rows"], g["queries"])
        s = np.sort(d, axis=1)
        assert (s[:, k - 1] == s[:, k]).any(), p
        if p.endswith("_far.npz"):  # the k-th best distance of query 0 is 64 W, in the selection's last bin
            far += 1
            assert g["rows"].shape[1] in (4, 16) and int(g["n_bits"]) == 64 * g["rows"].shape[1]
            bc.check_far(g["rows"], g["queries"], k, 0)
        big_head |= k > 16 and any(len(np.unique(d[q, :k])) < k for q in range(d.shape[0]))
    assert big_head and far == 2
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


def test_edge_inputs_every_width():
    """tests/bitvec_cases.py, the inputs of tests/test_bitvec_edges_gpu.py: each builder asserts what makes its input
    worth running, and the properties the GPU tests lean on are checked again here"""
    for W in range(1, 17):
        n_bits, rows, queries = bc.every_width(W)
        assert (n_bits + 63) // 64 == W and (n_bits % 64 != 0) == (W % 2 == 1)
        assert rows.shape == (1025, W) and queries.shape == (65, W)
        d0 = br.hamming_dists(rows, queries[:1])[0]
        assert bc.crosses(d0, 17)
        if W % 2:  # the noise counts: some distance of the whole rows is not the distance of the first n_bits bits
            keep = ~np.uint64((1 << (64 - n_bits % 64)) - 1)
            masked_r, masked_q = rows.copy(), queries.copy()
            masked_r[:, -1] &= keep
            masked_q[:, -1] &= keep
            assert not np.array_equal(br.hamming_dists(masked_r, masked_q[:2]), br.hamming_dists(rows, queries[:2]))


def test_edge_inputs_far_crowd():
    for W in range(1, 17):  # bitvec_select_m: every distance up to 64 W has a bin, and no M below it would do
        M = bc.select_m(W)
        assert 255 * M >= 64 * W > 255 * (M - 1)
    # the widths at which M steps up: there an M one less ends below 64 W and merges 64 W and 64 W - 1 in its last bin
    steps = [W for W in range(2, 17) if bc.select_m(W) > bc.select_m(W - 1)]
    assert steps == [4, 8, 12, 16] and all(255 * (bc.select_m(W) - 1) <= 64 * W - 1 for W in steps)
    assert set(bc.FAR_WIDTHS) >= {4, 8, 12, 16} and 1 in bc.FAR_WIDTHS and 3 in bc.FAR_WIDTHS
    for W in bc.FAR_WIDTHS:
        rows, queries = bc.far_crowd(W)
        s = np.sort(br.hamming_dists(rows, queries[:1])[0])
        assert s[0] == 64 * W - 3 and s[-1] == 64 * W
        ks = [bc.far_k(rows, queries, off) for off in (0, 1)]
        for k, off in zip(ks, (0, 1)):
            assert s[k - 1] == 64 * W - off == s[k]
    rows, queries = bc.far_crowd(8, n=1100)
    bc.check_far(rows, queries, 1024, 0)


def test_edge_inputs_seams_rerank_and_infinities():
    rows, base, want = bc.seam_query()
    assert rows.shape == (64, 1) and bc.distinct_answers(*want)
    nq = bc.QUERY_CHUNK + 5
    q = bc.periodic(base, nq)
    assert np.array_equal(q[bc.QUERY_CHUNK], base[bc.QUERY_CHUNK % bc.PERIOD]) and bc.QUERY_CHUNK % bc.PERIOD != 0
    at = bc.seam_window(nq)
    assert bc.QUERY_CHUNK - 1 in at and bc.QUERY_CHUNK in at and nq - 1 in at
    assert bc.distinct_answers(*bc.seam_rerank()[4])
    bc.small_chunks()
    assert bc.REFINER_MAX_DIM == 8176 and bc.RERANK_MAX_DIM == 14272 and bc.RERANK_DIMS[-1] == bc.REFINER_MAX_DIM
    assert [D % 4 for D in bc.RERANK_DIMS[:3]] == [1, 2, 0] and all(D > bc.RR_THREADS for D in bc.RERANK_DIMS)
    for D in bc.RERANK_DIMS[:4]:
        bc.rerank_edge(D)
    rows, queries, X, XQ, k, factor = bc.infinite_case()
    with np.errstate(over="ignore"):
        lab, dis = br.query_rerank(rows, queries, X, XQ, k, factor)
    assert (lab >= 0).all() and np.isinf(dis[:, k - 1]).all() and np.isfinite(dis[:, 0]).all()
    assert float(np.float32(3e19)) ** 2 > float(br.FLT_MAX)


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
