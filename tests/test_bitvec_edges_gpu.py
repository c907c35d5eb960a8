"""The Hamming engine at the edges tests/test_bitvec_gpu.py leaves out: every one of the sixteen scan kernels, k-th
best distances in the selection's top bins, the chunk seams of query and query_rerank, the rerank kernel's staging
loop past one step and its widest row, squared distances that overflow to +inf, and two streams through one engine.
The inputs come from tests/bitvec_cases.py, whose builders assert that each input does what it is there for
(tests/test_bitvec_ref_cpu.py runs them without a GPU); the checker is the restatement, tests/bitvec_ref.py.  Every
comparison is exact: labels and distances, ties included."""
import numpy as np
import pytest

import bitvec_cases as bc
import bitvec_ref as br
from vaq_amd import VaqBitVec, VaqHipError, VaqRefiner

pytestmark = pytest.mark.gpu


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


# ---- A: bitvec_scan_kernel<W> for every W: the register array, the uint4 loads and the scalar query loads are sized
# by W.  Two row tiles + 1 row, a query tile + 1 query, noise in the tail where W is odd, a crowd of ties at slot k
@pytest.mark.parametrize("W", range(1, 17))
def test_every_width(vaqlib, W):
    n_bits, rows, queries = bc.every_width(W)
    bv = VaqBitVec(0, n_bits)
    assert bv.W == W
    bv.set_rows(rows, id_base=1000)
    try:
        same(bv.query(queries, 17), br.query_sort(rows, queries, 17, id_base=1000))
    finally:
        bv.close()


# ---- B: rows at 64 W - 3 .. 64 W from query 0.  At W = 4, 8, 12, 16 the distance 64 W is the first past a multiple of
# 255: a histogram one M too small merges it with 64 W - 1 (the kernel clamps to its last bin) and picks wrong rows there
@pytest.mark.parametrize("W", bc.FAR_WIDTHS)
def test_far_crowd(vaqlib, W):
    rows, queries = bc.far_crowd(W)
    bv = VaqBitVec(0, 64 * W)
    bv.set_rows(rows, id_base=3)
    try:
        for off in (0, 1):  # the k-th best of query 0 is 64 W, then 64 W - 1; slot k inside the run either time
            k = bc.far_k(rows, queries, off)
            same(bv.query(queries, k), br.query_sort(rows, queries, k, id_base=3))
    finally:
        bv.close()


def test_far_crowd_full_head(vaqlib):
    """k = 1024 of 1100 rows at an M-step width: all of inv[] is in use and the k-th best distance is 64 W"""
    rows, queries = bc.far_crowd(8, n=1100)
    bc.check_far(rows, queries, 1024, 0)
    bv = VaqBitVec(0, 512)
    bv.set_rows(rows)
    try:
        same(bv.query(queries, 1024), br.query_sort(rows, queries, 1024))
    finally:
        bv.close()


# ---- C: chunk seams.  Queries repeat with period 7, which does not divide QUERY_CHUNK: an offset gone wrong behind
# the seam answers a query of another residue, and the seven answers are pairwise different
def check_periodic(got, want7, nq):
    idx = np.arange(nq) % bc.PERIOD
    assert np.array_equal(got[0], want7[0][idx])
    assert np.array_equal(got[1], want7[1][idx])


def test_query_across_the_query_chunk(vaqlib):
    nq = bc.QUERY_CHUNK + 5
    rows, base, want7 = bc.seam_query()
    queries = bc.periodic(base, nq)
    bv = VaqBitVec(0, 64)
    bv.set_rows(rows)
    try:
        got = bv.query(queries, 3)
    finally:
        bv.close()
    at = bc.seam_window(nq)
    same((got[0][at], got[1][at]), br.query_sort(rows, queries[at], 3))
    check_periodic(got, want7, nq)


def test_rerank_across_the_query_chunk(vaqlib):
    nq = bc.QUERY_CHUNK + 5
    rows, base, X, XQ7, want7 = bc.seam_rerank()
    queries, XQ = bc.periodic(base, nq), bc.periodic(XQ7, nq)
    bv = VaqBitVec(0, 64)
    bv.set_rows(rows)
    r = VaqRefiner(X.shape[1], 0)
    r.set_rows_u8(X)
    try:
        got = bv.query_rerank(queries, XQ, 2, 2, r)
    finally:
        r.close()
        bv.close()
    at = bc.seam_window(nq)
    same((got[0][at], got[1][at]), br.query_rerank(rows, queries[at], X, XQ[at], 2, 2))
    check_periodic(got, want7, nq)


def test_small_dist_chunks(vaqlib):
    """the inner chunk loop under the rerank (3 + 2 queries), and chunks of one query: dist_chunk_bytes below one
    query's matrix is the max(1, ...) branch"""
    rows, queries, X, XQ = bc.small_chunks()
    n_pad = (rows.shape[0] + 31) // 32 * 32
    want_q = br.query_sort(rows, queries, 17)
    want_r = br.query_rerank(rows, queries, X, XQ, 5, 3)
    bv = VaqBitVec(0, 64 * rows.shape[1])
    bv.set_rows(rows)
    r = VaqRefiner(X.shape[1], 0)
    r.set_rows_u8(X)
    try:
        bv.set_option("dist_chunk_bytes", 3 * n_pad * 2)
        same(bv.query_rerank(queries, XQ, 5, 3, r), want_r)
        bv.set_option("dist_chunk_bytes", 1)
        same(bv.query_rerank(queries, XQ, 5, 3, r), want_r)
        same(bv.query(queries, 17), want_q)
    finally:
        r.close()
        bv.close()


# ---- D: the rerank kernel past RR_THREADS columns (the staging loop's later steps), with a scalar remainder
# (D % 4 = 1, 2) and without, and at the widest row there is.  bitvec_rerank_max_dim() is 14272 floats, but a VaqRefiner
# takes rows of at most refine_rows_max_dim() = 8176 floats, so no row wider than that can reach the rerank: the
# launch at the limit is tested at 8176 (32 KiB of dynamic LDS beside the 8 KiB of candidate pairs), and 14273 is
# refused where the refiner is created, before any launch
@pytest.mark.parametrize("D", bc.RERANK_DIMS)
def test_rerank_wide_rows(vaqlib, D):
    rows, queries, Xf, XQf, Xb, XQb = bc.rerank_edge(D)
    k, factor = 5, 4
    bv = VaqBitVec(0, 128)
    bv.set_rows(rows, id_base=50)
    r = VaqRefiner(D, 0)
    try:
        r.set_rows(Xf, id_base=50)
        same(bv.query_rerank(queries, XQf, k, factor, r), br.query_rerank(rows, queries, Xf, XQf, k, factor, id_base=50))
        if D < bc.REFINER_MAX_DIM:
            want = br.query_rerank(rows, queries, Xb, XQb, k, factor, id_base=50)
            r.set_rows_u8(Xb, id_base=50)
            same(bv.query_rerank(queries, XQb, k, factor, r), want)
            r.set_rows(Xb.astype(np.float32), id_base=50)
            same(bv.query_rerank(queries, XQb, k, factor, r), want)
    finally:
        r.close()
        bv.close()


def test_rows_past_the_limit_are_refused(vaqlib):
    assert bc.REFINER_MAX_DIM == 8176 and bc.RERANK_MAX_DIM == 14272
    for D in (bc.REFINER_MAX_DIM + 1, bc.RERANK_MAX_DIM + 1):
        with pytest.raises(VaqHipError) as e:
            VaqRefiner(D, 0)
        assert e.value.code == -2


# ---- E: finite rows whose squared distance overflows.  The kernel marks invalid candidates with INFINITY too: a
# valid infinite candidate keeps its label, ranks by position among its equals, and its distance is inf, not FLT_MAX
def test_infinite_distances(vaqlib):
    rows, queries, X, XQ, k, factor = bc.infinite_case()
    with np.errstate(over="ignore"):
        want = br.query_rerank(rows, queries, X, XQ, k, factor, id_base=9)
    assert (want[0] >= 9).all() and np.isinf(want[1][:, -1]).all() and np.isfinite(want[1][:, 0]).all()
    bv = VaqBitVec(0, 128)
    bv.set_rows(rows, id_base=9)
    r = VaqRefiner(X.shape[1], 0)
    r.set_rows(X, id_base=9)
    try:
        got = bv.query_rerank(queries, XQ, k, factor, r)
    finally:
        r.close()
        bv.close()
    assert (got[0] >= 9).all()
    assert np.array_equal(np.isinf(got[1]), np.isinf(want[1])) and (got[1] != br.FLT_MAX).all()
    same(got, want)


# ---- F: the workspaces are shared by the callers' streams.  Four calls on two streams, interleaved, nothing
# synchronised until all are enqueued
def test_two_streams_share_one_engine(vaqlib):
    import torch
    rs = np.random.RandomState(61)
    n, W, D = 600, 2, 8
    rows = bc.near(rs, bc.words(rs, 1, W)[0], n, 9)
    X = rs.randint(0, 6, (n, D)).astype(np.uint8)
    calls = []  # per stream: (queries, XQ, k of query, k and factor of the rerank)
    for nq, kq, kr, factor in ((9, 20, 10, 4), (70, 7, 5, 3)):
        calls.append((bc.near(rs, rows[nq], nq, 5), rs.randint(0, 6, (nq, D)).astype(np.float32), kq, kr, factor))
    bv = VaqBitVec(0, 64 * W)
    bv.set_rows(rows)
    r = VaqRefiner(D, 0)
    r.set_rows_u8(X)
    dev = [(torch.from_numpy(q.view(np.int64)).cuda(), torch.from_numpy(xq).cuda()) for q, xq, _, _, _ in calls]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out_q, out_r = [None, None], [None, None]
    try:
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                out_q[i] = bv.query_device(dev[i][0], calls[i][2])
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                out_r[i] = bv.query_rerank_device(dev[i][0], dev[i][1], calls[i][3], calls[i][4], r)
        for s in streams:
            s.synchronize()
        for i, (q, xq, kq, kr, factor) in enumerate(calls):
            want_l, want_d = br.query_sort(rows, q, kq)
            assert np.array_equal(out_q[i][0].cpu().numpy(), want_l)
            assert np.array_equal(out_q[i][1].cpu().numpy(), want_d.astype(np.float32))
            same([t.cpu().numpy() for t in out_r[i]], br.query_rerank(rows, q, X, xq, kr, factor))
    finally:
        torch.cuda.synchronize()
        r.close()
        bv.close()
