"""The cluster form of the Hamming engine on the GPU (VaqBitVec.set_clusters, query_clusters, query_rerank_clusters over
vaqhip_bitvec_*_clusters) against the restatement, tests/bitvec_clusters_ref.py: labels and distances array_equal.

Bit rows differ from one base row in a handful of positions only, so the distances take few values and every cut falls
inside a crowd of equal distances that spans the head (the first k candidates), the others and several clusters.  The
select kernel walks tiles of 256 candidates; the plan ranks the centres 256 at a time and falls back to std::sort
wherever two centre distances are equal."""
import numpy as np
import pytest

import bitvec_clusters_ref as cr
from bitvec_cases import words
from vaq_amd import QueryMethod, VaqBitVec, VaqHipError, VaqRefiner

pytestmark = pytest.mark.gpu


def crowd(rs, n, W, nq, noise_tail=False):
    """(rows, queries): every row and query is one base row with bits turned in six fixed positions at most"""
    base = words(rs, 1, W)[0]
    spots = rs.choice(64 * W, 6, replace=False)

    def make(m):
        out = np.repeat(base[None, :], m, axis=0)
        for r in range(m):
            for b in spots[rs.randint(0, 2, 6) == 1]:
                out[r, b // 64] ^= np.uint64(1) << np.uint64(b % 64)
        if noise_tail:  # the low 13 bits of the last word lie past n_bits = 64 W - 13: they count all the same
            out[:, -1] ^= rs.randint(0, 2, m).astype(np.uint64) * np.uint64(0x1001)
        return out
    return make(n), make(nq)


def sizes_to_idx(rs, sizes):
    """a cluster index per row with the given cluster sizes, the rows of a cluster scattered"""
    return rs.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def centres_and_queries(rs, T, D, nq):
    return rs.standard_normal((T, D)).astype(np.float32), rs.standard_normal((nq, D)).astype(np.float32)


def run(n_bits, rows, queries, cen, idx, oq, k, atleast, id_base=0):
    bv = VaqBitVec(0, n_bits)
    bv.set_rows(rows, id_base=id_base)
    bv.set_clusters(cen, idx)
    got = bv.query_clusters(queries, oq, k, atleast_cluster=atleast)
    bv.close()
    want = cr.query_clusters(rows, queries, cen, idx, oq, k, atleast, id_base=id_base)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    return got


# 1200 rows: one empty cluster, one of 600 rows (more than two tiles), one of a single row
SIZES7 = [600, 0, 1, 257, 100, 200, 42]


@pytest.mark.parametrize("W", [1, 2, 3, 16])
def test_every_load_width(vaqlib, W):
    rs = np.random.RandomState(100 + W)
    rows, queries = crowd(rs, 1200, W, 9, noise_tail=W % 2 == 1)
    cen, oq = centres_and_queries(rs, 7, 5, 9)
    run(64 * W - 13 if W % 2 else 64 * W, rows, queries, cen, sizes_to_idx(rs, SIZES7), oq, 17, 1, id_base=1000)


@pytest.mark.parametrize("atleast", [1, 3, 7])
def test_atleast_cluster(vaqlib, atleast):
    rs = np.random.RandomState(7)
    rows, queries = crowd(rs, 1200, 2, 9)
    cen, oq = centres_and_queries(rs, 7, 5, 9)
    idx = sizes_to_idx(rs, SIZES7)
    got = run(128, rows, queries, cen, idx, oq, 17, atleast)
    if atleast == 7:  # every row is visited, in cluster order: the same distances as query, other rows among equals
        bv = VaqBitVec(0, 128)
        bv.set_rows(rows)
        lab, dis = bv.query(queries, 17)
        bv.close()
        assert np.array_equal(dis, got[1]) and not np.array_equal(lab, got[0])


# (n, k, cluster sizes): k = 1, 100, 1024 over 1100 rows; more slots than rows; a cluster of exactly k rows beside one
# of k + 1 (the walk stops at cum == k)
K_CASES = [(1100, 1, [500, 300, 300]), (1100, 100, [500, 300, 300]), (1100, 1024, [500, 300, 300]),
           (700, 1024, [400, 0, 300]), (400, 100, [100, 101, 99, 100])]


@pytest.mark.parametrize("n,k,sizes", K_CASES)
def test_k_and_the_walk(vaqlib, n, k, sizes):
    rs = np.random.RandomState(n + k)
    rows, queries = crowd(rs, n, 2, 8)
    cen, oq = centres_and_queries(rs, len(sizes), 3, 8)
    oq[:len(sizes)] = cen  # query c stands on centre c: each cluster is some query's first
    run(128, rows, queries, cen, sizes_to_idx(rs, sizes), oq, k, 1)


@pytest.mark.parametrize("T,ties", [(1, True), (17, True), (300, True), (300, False)])
def test_centre_order(vaqlib, T, ties):
    """equal centre distances: duplicated centres, and pairs mirrored about query 0 (the same float distance, bit for
    bit); the order inside a run is std::sort's.  T = 17 passes the introsort's threshold, T = 300 the ranking stride."""
    rs = np.random.RandomState(T)
    D = 4
    cen, oq = centres_and_queries(rs, T, D, 6)
    if ties and T > 1:
        oq[0] = 0
        cen[1::4] = cen[0::4][:len(cen[1::4])]  # duplicates
        cen[2::4] = -cen[3::4][:len(cen[2::4])]  # mirrored about the origin, query 0
        assert len(np.unique(cr.br.euclidean_no_sqrt(oq[0], cen))) < T // 2 + 2
    else:
        assert all(len(np.unique(cr.br.euclidean_no_sqrt(q, cen))) == T for q in oq)
    rows, queries = crowd(rs, 900, 2, 6)
    idx = rs.randint(0, T, 900).astype(np.int32)
    run(128, rows, queries, cen, idx, oq, 17, min(T, 5))


@pytest.mark.parametrize("D", [7, 128])
def test_rerank(vaqlib, D):
    rs = np.random.RandomState(D)
    rows, queries = crowd(rs, 1200, 2, 5)
    idx = sizes_to_idx(rs, SIZES7)
    X = rs.randint(0, 3, (1200, D)).astype(np.uint8)  # a narrow range: equal squared distances everywhere
    XQ = rs.randint(0, 3, (5, D)).astype(np.float32)
    cen = X[rs.choice(1200, 7, replace=False)].astype(np.float32)
    want = cr.query_rerank_clusters(rows, queries, cen, idx, X, XQ, 20, 3, 2, id_base=1000)
    bv = VaqBitVec(0, 128)
    bv.set_rows(rows, id_base=1000)
    bv.set_clusters(cen, idx)
    for as_bytes in (True, False):
        r = VaqRefiner(D, 0)
        if as_bytes:
            r.set_rows_u8(X, id_base=1000)
        else:
            r.set_rows(X.astype(np.float32), id_base=1000)
        lab, dis = bv.query_rerank_clusters(queries, XQ, 20, 3, r, atleast_cluster=2)
        assert np.array_equal(lab, want[0])
        assert np.array_equal(dis, want[1])
        r.close()
    bv.close()


def test_device_forms_on_another_stream(vaqlib):
    import torch
    rs = np.random.RandomState(5)
    rows, queries = crowd(rs, 1200, 2, 9)
    idx = sizes_to_idx(rs, SIZES7)
    X = rs.randint(0, 3, (1200, 8)).astype(np.uint8)
    XQ = rs.randint(0, 3, (9, 8)).astype(np.float32)
    cen = rs.standard_normal((7, 8)).astype(np.float32)
    bv = VaqBitVec(0, 128)
    bv.set_rows(rows)
    bv.set_clusters(cen, idx)
    r = VaqRefiner(8, 0)
    r.set_rows_u8(X)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(queries.view(np.int64)).cuda()
        doq = torch.from_numpy(XQ).cuda()
        out = (torch.empty((9, 17), dtype=torch.int32, device="cuda"), torch.empty((9, 17), dtype=torch.float32, device="cuda"))
        lab, dis = bv.query_clusters_device(dq, doq, 17, atleast_cluster=2, out=out)
        rl, rd = bv.query_rerank_clusters_device(dq, doq, 10, 4, r, atleast_cluster=2)
    s.synchronize()
    assert lab is out[0] and dis is out[1]
    want = cr.query_clusters(rows, queries, cen, idx, XQ, 17, 2)
    assert np.array_equal(lab.cpu().numpy(), want[0])
    assert np.array_equal(dis.cpu().numpy(), want[1].astype(np.float32))
    want = cr.query_rerank_clusters(rows, queries, cen, idx, X, XQ, 10, 4, 2)
    assert np.array_equal(rl.cpu().numpy(), want[0])
    assert np.array_equal(rd.cpu().numpy(), want[1])
    r.close()
    bv.close()


@pytest.mark.parametrize("case,code", [("before_set_clusters", -7), ("after_add_rows", -7), ("clust_idx_range", -1),
                                       ("atleast_0", -1), ("atleast_T_plus_1", -1), ("method_heap", -2)])
def test_refusals(vaqlib, case, code):
    rs = np.random.RandomState(9)
    rows, queries = crowd(rs, 300, 1, 2)
    cen, oq = centres_and_queries(rs, 4, 3, 2)
    idx = rs.randint(0, 4, 300).astype(np.int32)
    lib = vaqlib
    bv = VaqBitVec(0, 64)
    bv.set_rows(rows)
    lab, dis = np.empty((2, 3), np.int32), np.empty((2, 3), np.float32)

    def raw(method=QueryMethod.Sort, atleast=1):  # the C entry itself: the adapter's own refusals are not in the way
        return lib.vaqhip_bitvec_query_clusters(bv._h, queries.ctypes.data, oq.ctypes.data, 2, 3, method, atleast,
                                                lab.ctypes.data, dis.ctypes.data)
    if case == "clust_idx_range":
        bad = idx.copy()
        bad[17] = 4
        assert lib.vaqhip_bitvec_set_clusters(bv._h, cen.ctypes.data, 4, 3, bad.ctypes.data) == code
        with pytest.raises(VaqHipError) as e:
            bv.set_clusters(cen, bad)
        assert e.value.code == code
    elif case == "before_set_clusters":
        assert raw() == code
    else:
        bv.set_clusters(cen, idx)
        assert raw() == 0
        if case == "after_add_rows":
            bv.add_rows(rows[:1])
            assert raw() == code
            with pytest.raises(VaqHipError) as e:
                bv.query_clusters(queries, oq, 3)
            assert e.value.code == code
        else:
            got = raw(**{"atleast_0": dict(atleast=0), "atleast_T_plus_1": dict(atleast=5),
                         "method_heap": dict(method=QueryMethod.Heap)}[case])
            assert got == code
    bv.close()
