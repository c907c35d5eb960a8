"""What the cases of tests/test_bucket_major_edges_gpu.py must be for their tests to reach the branches they
name.  No GPU: the builders are plain numpy, the distances are the CPU oracle's.  These are conditions on the
inputs, not measurements of the library; a changed seed that breaks one fails here instead of quietly emptying
a GPU test."""
import numpy as np
import pytest

import test_bucket_major_edges_gpu as E


def luts(oracle, c):
    """The oracle's tables of every query: (nq, M, 256)."""
    Xp = oracle.project(c["X"], c["eig"]) if c["eig"] is not None else c["X"]
    return np.stack([oracle.create_lut(Xp[q], c["cents"], 8) for q in range(Xp.shape[0])])


@pytest.mark.parametrize("M", [8, 16, 32])
def test_sparse_case_has_empty_and_tiny_buckets(M):
    """Case 1 (and case 9's 33-query variant)."""
    for c in (E.sparse_case(M), E.sparse_case(M, nq=33)):
        codes = c["codes"]
        assert codes.shape == (3001, M) and codes.max() < 256
        rows = np.bincount(E.bucket_ids(codes, 10), minlength=1024)
        assert rows.sum() == 3001 and len(rows) == 1024
        assert (rows == 0).sum() > 10 and (rows == 1).sum() > 10 and ((rows > 0) & (rows < 64)).sum() > 900
        runs = np.bincount((codes[:, 0].astype(np.int64) << 8) | codes[:, 1], minlength=65536)
        assert (runs == 0).sum() > 60000          # most runs are empty ...
        assert (runs > 1).sum() > 0               # ... and duplicated rows share one
        # at 7, 11 and 12 bits (the refusals) the key is a different one: 128 / 2048 / 4096 buckets
        assert len(np.unique(codes[:, 0] >> 1)) == 128


def test_skewed_case_sizes_and_boot_clipping(oracle):
    """Case 2: the four bucket sizes; every query's nearest bucket is the one it was aimed at; among the queries
    of the large bucket one has its nearest run start in the last 4096 rows (the short tail) and one earlier
    (the plain clip); at bucket_bits 9 the samples lie between k and 4096 rows."""
    c = E.skewed_case()
    codes = c["codes"]
    assert codes.shape[0] == 6000
    rows = np.bincount(E.bucket_ids(codes, 8), minlength=256)
    assert tuple(rows[list(E.SKEW_FIRST)]) == E.SKEW_SIZES == (1, 63, 65, 5871) and (rows > 0).sum() == 4
    assert rows.max() > E.BM_BOOT_ROWS
    lut = luts(oracle, c)
    short_tail = plain_clip = 0
    for q in range(12):
        b, n, off = E.nearest_run_start(lut[q], codes, 8)
        assert b == E.SKEW_FIRST[q % 4] and n == E.SKEW_SIZES[q % 4], q
        if n > E.BM_BOOT_ROWS:
            short_tail += n - off < E.BM_BOOT_ROWS
            plain_clip += n - off >= E.BM_BOOT_ROWS and off > 0
    assert short_tail >= 1 and plain_clip >= 1, (short_tail, plain_clip)
    # query 3: its nearest run is the large bucket's last, shorter than k = 100; fewer than 256 rows of the index
    # lie at or below the k-th distance of the runs that are wholly inside the bucket's last 4096 rows (a subset
    # of the sample, whatever the order inside a run: the sample's own k-th distance is no larger)
    q, k = E.SKEW_TAIL_QUERY, 100
    b, n, off = E.nearest_run_start(lut[q], codes, 8)
    assert b == E.SKEW_FIRST[3] and 0 < n - off < k
    inside = codes[E.bucket_ids(codes, 8) == b, 1].astype(np.int64)
    first_whole = min(j for j in np.unique(inside) if (inside < j).sum() >= n - E.BM_BOOT_ROWS)
    ad = oracle.all_dists(lut[q], codes)
    part = ad[(E.bucket_ids(codes, 8) == b) & (codes[:, 1] >= first_whole)]
    assert k < len(part) <= E.BM_BOOT_ROWS
    assert k <= (ad <= np.sort(part)[k - 1]).sum() < 256
    # query 12: some empty bucket has a smaller key than its nearest non-empty one, the large bucket
    q = E.SKEW_EMPTY_QUERY
    b, n, _ = E.nearest_run_start(lut[q], codes, 8)
    assert b == E.SKEW_FIRST[3] and n == E.SKEW_SIZES[3]
    key = lut[q][0].view(np.uint32) & ~np.uint32(255)
    assert (key[rows == 0] < key[b]).sum() >= 1
    # sample sizes at bucket_bits 8: below k = 10, between 10 and 100, above 100 and clipped
    assert {1, 63, 65} <= {E.SKEW_SIZES[q % 4] for q in range(12)} and lut.shape[0] == 13
    rows9 = np.bincount(E.bucket_ids(codes, 9), minlength=512)
    assert 100 < rows9.max() < E.BM_BOOT_ROWS and (rows9 == 1).sum() == 1
    sizes9 = {E.nearest_run_start(lut[q], codes, 9)[1] for q in range(lut.shape[0])}
    assert min(sizes9) < 10 and max(sizes9) > 100, sizes9


def test_small_cases_have_fewer_rows_than_k():
    """Case 3: N < k, and 300 rows against k = 256 (nearly every row is wanted)."""
    assert [n for n, _, _ in E.SMALL_N] == [1, 7, 40, 300]
    for N, M, bucket_bits in E.SMALL_N:
        c = E.small_case(N, M)
        assert c["codes"].shape == (N, M) and M in (8, 16, 32) and bucket_bits in (8, 9, 10)
        assert E.SMALL_K[N] and all(k <= 256 and (N < k or N == 300) for k in E.SMALL_K[N])
    assert E.SMALL_K[300] == (256,) and E.SMALL_K[1] == E.SMALL_K[7] == E.SMALL_K[40] == (100, 256)


def test_nonfinite_case_rows(oracle):
    """Case 6: the oracle itself gives the marked rows +inf and never returns them; fewer finite rows than the
    largest k; the three non-finite queries get nothing at all."""
    c = E.nonfinite_case()
    codes = c["codes"]
    assert c["eig"] is None and codes.shape == (3001, 8)
    bad = (codes[:, 0] == E.NONFINITE_FIRST) | (codes[:, 1] == E.NONFINITE_SECOND)
    both = (codes[:, 0] == E.NONFINITE_FIRST) & (codes[:, 1] == E.NONFINITE_SECOND)
    finite = int((~bad).sum())
    assert bad.sum() > 0 and both.sum() > 0 and max(E.NONFINITE_K) == 256
    assert min(E.NONFINITE_K) < 100 < finite < 256
    lut = luts(oracle, c)
    good_q = [0, 4, 5, 6]
    assert np.all(np.isposinf(lut[good_q, 0, E.NONFINITE_FIRST])) and np.all(np.isposinf(lut[good_q, 1, E.NONFINITE_SECOND]))
    assert np.all(np.isnan(lut[1])) and np.all(np.isposinf(lut[2, 0])) and np.all(np.isposinf(lut[3, 2]))
    for q in (0, 3):  # (query 3's bucket bounds are finite: only its rows are not)
        assert np.all(np.isfinite(np.delete(lut[q, 0], E.NONFINITE_FIRST)))
    ad = np.stack([oracle.all_dists(lut[q], codes) for q in range(lut.shape[0])])
    for q in good_q:
        assert np.array_equal(np.isposinf(ad[q]), bad) and np.all(np.isfinite(ad[q][~bad]))
    assert np.all(np.isnan(ad[1])) and np.all(np.isposinf(ad[2])) and np.all(np.isposinf(ad[3]))
    for k in E.NONFINITE_K:
        o_lab, o_dis = oracle.search(c["X"], c["cents"], codes, k, max_bits=8, projected=True)
        assert np.all(o_lab[1:4] == -1) and np.all(o_dis[1:4] == E.FLT_MAX)
        for q in good_q:
            assert not np.any(bad[o_lab[q][o_lab[q] >= 0]])
            assert (o_lab[q] >= 0).sum() == min(k, finite)
    # buckets with an infinite bound: one at 8 bits, four at 10
    assert len(np.unique(E.bucket_ids(codes[codes[:, 0] == E.NONFINITE_FIRST], 10))) == 4


@pytest.mark.parametrize("k", E.TIED_K)
def test_tied_case_ties_at_k_for_every_query(oracle, k):
    """Case 7: the k-th and (k+1)-th oracle distances are equal for every query, and for some query the tied
    distance is the 5000-row block's: more equal rows than any candidate buffer of the test holds."""
    c = E.tied_case()
    codes = c["codes"]
    assert codes.shape == (E.TIED_N, 8)
    vecs, counts = np.unique(codes, axis=0, return_counts=True)
    assert len(vecs) == E.TIED_DISTINCT + 1 and counts.max() == E.TIED_BLOCK > 64
    block = np.nonzero((codes == vecs[np.argmax(counts)]).all(axis=1))[0]
    assert block[0] < 10 and block[-1] > E.TIED_N - 10 and np.any(np.diff(block) > 1)  # scattered over the labels
    lut = luts(oracle, c)
    in_block = 0
    for q in range(lut.shape[0]):
        d = np.sort(oracle.all_dists(lut[q], codes))
        assert d[k - 1] == d[k], (q, d[k - 2:k + 2])
        in_block += int((d == d[k - 1]).sum() >= E.TIED_BLOCK)
    assert in_block >= 1


def test_growth_case_fills_an_empty_bucket():
    """Case 9."""
    c, more, b = E.growth_case()
    assert c["X"].shape[0] == 33 and more.shape == (64, 16)
    assert not np.any(E.bucket_ids(c["codes"], 10) == b) and np.all(E.bucket_ids(more, 10) == b)
    assert len(np.unique(more[:, 1])) > 8  # several runs of that bucket
