"""The cluster form of the Hamming engine at the edges tests/test_bitvec_clusters_gpu.py leaves out: every one of the
sixteen select kernels, cuts in the far bins and in a middle thread's bins, the plan kernel at its stride edge and its
limits of T and D, centre distances that must not fuse, that are +inf or NaN, the two query-chunk loops of the host,
a handle whose cluster state is replaced or dropped, and fixtures the compiled reference answered.  The inputs come
from tests/bitvec_clusters_cases.py, whose builders assert that each input does what it is there for
(tests/test_bitvec_clusters_cpu.py runs them without a GPU); the checker is the restatement,
tests/bitvec_clusters_ref.py.  Every comparison is exact: labels and distances, ties included."""
import glob
import os

import numpy as np
import pytest

import bitvec_cases as bc
import bitvec_clusters_cases as cc
import bitvec_clusters_ref as cr
from vaq_amd import QueryMethod, VaqBitVec, VaqHipError, VaqRefiner

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hamming")


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


def engine(n_bits, rows, cen, idx, id_base=0):
    bv = VaqBitVec(0, n_bits)
    bv.set_rows(rows, id_base=id_base)
    bv.set_clusters(cen, idx)
    return bv


def check(n_bits, rows, queries, cen, idx, oq, runs, id_base=0):
    """query_clusters on one engine for every (k, atleast) of runs, against the restatement"""
    with np.errstate(over="ignore", invalid="ignore"):
        wants = [cr.query_clusters(rows, queries, cen, idx, oq, k, atleast, id_base=id_base) for k, atleast in runs]
    bv = engine(n_bits, rows, cen, idx, id_base)
    try:
        for (k, atleast), want in zip(runs, wants):
            same(bv.query_clusters(queries, oq, k, atleast_cluster=atleast), want)
    finally:
        bv.close()
    return wants


# ---- A: cluster_select_kernel<W> for every W: the register array, the uint2 / uint4 loads, BINS = 64 W + 1 and PER are
# sized by W.  Clusters of 0, 1, 255, 256, 257 and 513 rows; half the rows at distances round 32 W
@pytest.mark.parametrize("W", range(1, 17))
def test_every_width(vaqlib, W):
    n_bits, rows, queries, cen, idx, oq = cc.every_width(W)
    check(n_bits, rows, queries, cen, idx, oq, [(cc.K_A, cc.ATLEAST_A)], id_base=cc.ID_BASE_A)


# ---- B: query 0 sees only the distances 64 W - 3 .. 64 W: its cut lies in the last bin, then in the one before, which
# belong to the last thread with a bin (PER = 1, 1, 2, 3, 4, 5 here); query 1's cut lies near 32 W in a middle thread's
# bins, so the prefix over the 256 threads decides.  Every cluster walked, then a strict subset
@pytest.mark.parametrize("W", bc.FAR_WIDTHS)
def test_far_bins(vaqlib, W):
    case = cc.far_clusters(W)
    rows, queries, cen, idx, oq = case
    runs = [(cc.far_k(case, off, atleast), atleast) for atleast in (len(cen), 1) for off in (0, 1)]
    for (k, atleast), off in zip(runs, (0, 1, 0, 1)):
        cc.check_far(case, k, off, atleast)
    check(64 * W, rows, queries, cen, idx, oq, runs, id_base=cc.ID_BASE_B)


def test_far_bins_full_head(vaqlib):
    """k = 1024 of 1100 rows at W = 8: inv[], keys[] and the bitonic sort at their full size, P = 1024"""
    rows, queries, cen, idx, oq, k = cc.full_head()
    check(64 * rows.shape[1], rows, queries, cen, idx, oq, [(k, len(cen))])


# ---- C: the plan.  T at the per-thread stride edge and at its limit, D at its limits, either term sizing the first LDS
# region; all distances distinct (the ranking) and tied (the one-thread std::sort); empty clusters among the nearest
@pytest.mark.parametrize("T,D,nq", cc.PLAN_SHAPES)
def test_plan_shapes(vaqlib, T, D, nq):
    rows, queries, cen, idx, oq, atleast = cc.plan_shape(T, D, nq, False)
    check(128, rows, queries, cen, idx, oq, [(cc.K_C, atleast)])


@pytest.mark.parametrize("T,D,nq", cc.PLAN_TIE_SHAPES)
def test_plan_shapes_with_ties(vaqlib, T, D, nq):
    rows, queries, cen, idx, oq, atleast = cc.plan_shape(T, D, nq, True)
    check(128, rows, queries, cen, idx, oq, [(cc.K_C, atleast)])


@pytest.mark.parametrize("seed", range(4))
def test_plan_sum_does_not_fuse(vaqlib, seed):
    """two centres whose order under acc = fma(t, t, acc) is not their order under the reference's three roundings:
    each cluster alone holds k rows, so the labels of query 0 say which was visited"""
    rows, queries, cen, idx, oq = cc.fuse_sensitive(seed)
    want, = check(64, rows, queries, cen, idx, oq, [(cc.K_C, 1)])
    fused = cr.query_clusters(rows, queries, cen, idx, oq, cc.K_C, 1, dist=cc.euclidean_fused)
    assert not np.array_equal(want[0][0], fused[0][0])


@pytest.mark.parametrize("kind", cc.NONFINITE)
def test_plan_nonfinite_distances(vaqlib, kind):
    """+inf from finite inputs: several centres tie there and the walk reaches them.  NaN: std::sort is outside what
    C++ defines; the answer is the restated sort's (tests/cpp/cluster_sort_test.cpp holds the device's sort, built for
    the host, against the checker's on these arrays)"""
    rows, queries, cen, idx, oq, k, atleast = cc.nonfinite(kind)
    check(128, rows, queries, cen, idx, oq, [(k, atleast)])


# ---- D: the host's seams
def test_small_dist_chunks(vaqlib):
    """clusters_enqueue's chunk loop: 3 + 2 queries, then one query a chunk (the max(1, ...) branch), under the plain
    form and under the rerank's own loop"""
    rows, queries, X, XQ, cen, idx = cc.small_chunks()
    want_q = cr.query_clusters(rows, queries, cen, idx, XQ, 17, 2)
    want_r = cr.query_rerank_clusters(rows, queries, cen, idx, X, XQ, 5, 3, 2)
    bv = engine(64 * rows.shape[1], rows, cen, idx)
    r = VaqRefiner(X.shape[1], 0)
    r.set_rows_u8(X)
    try:
        for chunk_bytes in (3 * cc.PER_QUERY_BYTES(len(cen)), 1):
            bv.set_option("dist_chunk_bytes", chunk_bytes)
            same(bv.query_clusters(queries, XQ, 17, atleast_cluster=2), want_q)
            same(bv.query_rerank_clusters(queries, XQ, 5, 3, r, atleast_cluster=2), want_r)
    finally:
        r.close()
        bv.close()


def check_periodic(got, want7, nq):
    at = np.arange(nq) % bc.PERIOD
    assert np.array_equal(got[0], want7[0][at])
    assert np.array_equal(got[1], want7[1][at])


@pytest.mark.parametrize("form", ["query_clusters", "query_rerank_clusters"])
def test_across_the_query_chunk(vaqlib, form):
    """nq = QUERY_CHUNK + 5, bit queries and raw queries of period 7: behind the seam d_bq, d_oq, d_labels and d_dist are
    offset each by its own stride; the answers follow both kinds of query, so each wrong offset changes them"""
    nq = bc.QUERY_CHUNK + 5
    rows, base, X, XQ7, cen, idx, want7, want7_rr = cc.seam()
    queries, XQ = bc.periodic(base, nq), bc.periodic(XQ7, nq)
    at = bc.seam_window(nq)
    bv = engine(64, rows, cen, idx)
    r = VaqRefiner(X.shape[1], 0)
    r.set_rows_u8(X)
    try:
        if form == "query_clusters":
            got = bv.query_clusters(queries, XQ, 3)
            want7, window = want7, cr.query_clusters(rows, queries[at], cen, idx, XQ[at], 3, 1)
        else:
            got = bv.query_rerank_clusters(queries, XQ, 2, 2, r)
            want7, window = want7_rr, cr.query_rerank_clusters(rows, queries[at], cen, idx, X, XQ[at], 2, 2, 1)
    finally:
        r.close()
        bv.close()
    same((got[0][at], got[1][at]), window)
    check_periodic(got, want7, nq)


# ---- E: state
def test_set_clusters_again_on_one_handle(vaqlib):
    """another T (300, 3, 300), another D, fewer rows with other cluster sizes: the buffers are reused through ensure,
    and each answer is that of a fresh handle given the same final state"""
    steps, queries, oq = cc.state_steps()
    bv = VaqBitVec(0, 128)
    held = None
    try:
        for rows, cen, idx in steps:
            if rows is not None:
                bv.set_rows(rows, id_base=5)
                held = rows
            bv.set_clusters(cen, idx)
            atleast = min(3, len(cen))
            got = bv.query_clusters(queries, oq[cen.shape[1]], 17, atleast_cluster=atleast)
            same(got, cr.query_clusters(held, queries, cen, idx, oq[cen.shape[1]], 17, atleast, id_base=5))
            fresh = engine(128, held, cen, idx, id_base=5)
            try:
                same(got, fresh.query_clusters(queries, oq[cen.shape[1]], 17, atleast_cluster=atleast))
            finally:
                fresh.close()
    finally:
        bv.close()


DROPS = ["set_rows", "set_rows_device", "encode_set_rows", "encode_set_rows_u8", "encode_add_rows", "encode_add_rows_u8",
         "encode_from_refiner"]


@pytest.mark.parametrize("how", DROPS)
def test_what_drops_the_cluster_state(vaqlib, how):
    """whatever replaces or appends rows: the C entry answers VAQHIP_ESTATE until the next set_clusters, and right
    answers behind it"""
    import torch
    rs = np.random.RandomState(len(how))
    rows, queries = cc.crowd(rs, 300, 1, 2)
    cen = rs.standard_normal((4, 3)).astype(np.float32)
    oq = rs.standard_normal((2, 3)).astype(np.float32)
    Xf = rs.standard_normal((300, 64)).astype(np.float32)
    Xb = rs.randint(0, 256, (300, 64)).astype(np.uint8)
    bv = VaqBitVec(0, 64)
    bv.set_encoder(64)  # one sign bit per dimension
    bv.set_rows(rows)
    lab, dis = np.empty((2, 3), np.int32), np.empty((2, 3), np.float32)

    def raw():  # the C entry itself
        return vaqlib.vaqhip_bitvec_query_clusters(bv._h, queries.ctypes.data, oq.ctypes.data, 2, 3, QueryMethod.Sort, 1,
                                                   lab.ctypes.data, dis.ctypes.data)
    r = None
    try:
        bv.set_clusters(cen, rs.randint(0, 4, 300).astype(np.int32))
        assert raw() == 0
        if how == "set_rows":
            held = rows[:200]
            bv.set_rows(held)
        elif how == "set_rows_device":
            held = rows[:200]
            bv.set_rows(torch.from_numpy(held.view(np.int64)).cuda())
        elif how == "encode_set_rows":
            held = bv.encode(Xf[:200])
            bv.set_rows_encoded(Xf[:200])
        elif how == "encode_set_rows_u8":
            held = bv.encode(Xb[:200])
            bv.set_rows_encoded(Xb[:200])
        elif how == "encode_add_rows":
            held = np.vstack([rows, bv.encode(Xf[:7])])
            bv.add_rows_encoded(Xf[:7])
        elif how == "encode_add_rows_u8":
            held = np.vstack([rows, bv.encode(Xb[:7])])
            bv.add_rows_encoded(Xb[:7])
        else:
            held = bv.encode(Xf[:200])
            r = VaqRefiner(64, 0)
            r.set_rows(Xf[:200])
            bv.encode_from_refiner(r)
        assert raw() == -7
        with pytest.raises(VaqHipError) as e:
            bv.query_clusters(queries, oq, 3)
        assert e.value.code == -7
        assert len(bv) == held.shape[0]
        idx = rs.randint(0, 4, held.shape[0]).astype(np.int32)
        bv.set_clusters(cen, idx)
        assert raw() == 0
        same(bv.query_clusters(queries, oq, 3, atleast_cluster=2), cr.query_clusters(held, queries, cen, idx, oq, 3, 2))
    finally:
        if r is not None:
            r.close()
        bv.close()


def test_refiner_of_another_dimension_is_refused(vaqlib):
    rs = np.random.RandomState(4)
    rows, queries = cc.crowd(rs, 300, 1, 2)
    bv = engine(64, rows, rs.standard_normal((4, 3)).astype(np.float32), rs.randint(0, 4, 300).astype(np.int32))
    r = VaqRefiner(5, 0)
    r.set_rows(rs.standard_normal((300, 5)).astype(np.float32))
    oq = rs.standard_normal((2, 3)).astype(np.float32)
    lab, dis = np.empty((2, 3), np.int32), np.empty((2, 3), np.float32)
    try:
        rc = vaqlib.vaqhip_bitvec_query_rerank_clusters(bv._h, r._h, queries.ctypes.data, oq.ctypes.data, 2, 3, 2, 1,
                                                        lab.ctypes.data, dis.ctypes.data)
        assert rc == -1 and b"D=5" in vaqlib.vaqhip_last_error() and b"D=3" in vaqlib.vaqhip_last_error()
        with pytest.raises(VaqHipError) as e:
            bv.query_rerank_clusters(queries, oq, 3, 2, r)
        assert e.value.code == -1
    finally:
        r.close()
        bv.close()


def test_engine_with_no_rows(vaqlib):
    """include/vaqhip.h: an engine with no rows takes set_clusters (no cluster index is read) and answers every slot
    -1 / FLT_MAX, the rerank form too"""
    rs = np.random.RandomState(6)
    cen = rs.standard_normal((5, 3)).astype(np.float32)
    oq = rs.standard_normal((4, 3)).astype(np.float32)
    queries = bc.words(rs, 4, 1)
    bv = VaqBitVec(0, 64)
    r = VaqRefiner(3, 0)
    try:
        assert len(bv) == 0
        assert vaqlib.vaqhip_bitvec_set_clusters(bv._h, cen.ctypes.data, 5, 3, None) == 0
        bv.set_clusters(cen, np.zeros(0, np.int32))
        lab, dis = bv.query_clusters(queries, oq, 7, atleast_cluster=5)
        assert (lab == -1).all() and (dis == 0xffffffff).all()
        lab, dis = bv.query_rerank_clusters(queries, oq, 7, 3, r)
        assert (lab == -1).all() and (dis == np.finfo(np.float32).max).all()
        # rows arrive: the state is dropped like any other, and a new one answers
        rows = cc.crowd(rs, 50, 1, 1)[0]
        bv.set_rows(rows)
        with pytest.raises(VaqHipError) as e:
            bv.query_clusters(queries, oq, 7)
        assert e.value.code == -7
        idx = rs.randint(0, 5, 50).astype(np.int32)
        bv.set_clusters(cen, idx)
        same(bv.query_clusters(queries, oq, 7, atleast_cluster=2), cr.query_clusters(rows, queries, cen, idx, oq, 7, 2))
    finally:
        r.close()
        bv.close()


# ---- F: the fixtures the compiled reference's KNNFromDists answered (tests/golden/hamming/README.md)
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "clusters_*.npz"))), ids=lambda p: os.path.basename(p)[:-4])
def test_fixture(vaqlib, path):
    g = np.load(path)
    k, atleast = int(g["k"]), int(g["atleast"])
    bv = engine(int(g["n_bits"]), g["rows"], g["centroids"], g["clust_idx"])
    r = None
    try:
        if "factor" in g:
            r = VaqRefiner(g["X"].shape[1], 0)
            r.set_rows_u8(g["X"])
            ham, _ = bv.query_clusters(g["queries"], g["XQ"], int(g["k_walk"]), atleast_cluster=atleast)
            assert np.array_equal(ham, g["hamming_labels"])
            got = bv.query_rerank_clusters(g["queries"], g["XQ"], k, int(g["factor"]), r, atleast_cluster=atleast)
        else:
            got = bv.query_clusters(g["queries"], g["XQ"], k, atleast_cluster=atleast)
    finally:
        if r is not None:
            r.close()
        bv.close()
    same(got, (g["labels"], g["dists"]))


def test_fixtures_exist():
    assert len(glob.glob(os.path.join(GOLD, "clusters_*.npz"))) >= 2
