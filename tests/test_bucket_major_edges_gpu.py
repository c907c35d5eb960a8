"""The bucket-major rounds (vaq_amd/csrc/vaq_scan_bm.hip: mark, boot, order, fill, sort, scan, select) where
they are fragile rather than fast: a few thousand rows over 256-1024 buckets, so that buckets and runs are
empty or hold a handful of rows, N < k, a label offset, bucket bounds that are not finite, query counts below
the group size, thousands of identical rows against a candidate buffer of one slot, and the settings the plan
must refuse.  tests/test_bucket_major_gpu.py covers the same kernels with 260 k - 1.5 M uniformly drawn rows.

Reference: the CPU oracle on the unpacked uint16 codes.  Every result of the rounds is checked twice: against
the oracle (distances bit for bit, labels under the tie contract of helpers.assert_topk_matches) and bit for
bit -- labels and distance bits -- against option bucket_major = 0 on the same index.  No tolerance anywhere.
A run that must take the rounds asserts last_timing()["bucket_major"] == 1, a refused one == 0.

The case builders need no GPU; tests/test_bucket_major_edges_cpu.py asserts of each what makes it reach its
branch (empty buckets, the four bucket sizes, N < k, ...), so that a changed seed cannot empty a case."""
import numpy as np
import pytest

from helpers import assert_topk_matches, make_case
from test_bucket_major_gpu import make_index, oracle_all_dists, run

pytestmark = pytest.mark.gpu

BM_BOOT_ROWS = 4096  # rows of the sample behind a sampled threshold (vaq_scan_bm.hip)
FLT_MAX = np.finfo(np.float32).max


def dims(M):
    return 8 * M if M <= 16 else 4 * M


def bucket_ids(codes, bucket_bits):
    """Bucket of every row for all-8-bit codes and 8 <= bucket_bits <= 12: the first code, continued by the
    top bits of the second."""
    bt = bucket_bits - 8
    return (codes[:, 0].astype(np.int64) << bt) | (codes[:, 1].astype(np.int64) >> (8 - bt))


def opts(boot, rnd, qb, nw, runs, cap=0):
    return dict(bm_boot=boot, bm_units=1, bm_round=rnd, bm_queries_per_group=qb, bm_waves=nw, bm_runs=runs,
                bm_candidates=cap)


# The reduced option sweep: a best-first pass A of one work unit / a sampled threshold; the middle round absent,
# of 1 bucket, of 6; 2 / 4 / automatic queries per group; 4 / 16 / automatic waves; the runs inside a bucket
# skipped or ignored.  Every value of every option occurs with both forms of pass A.
SWEEP = [opts(0, 6, 0, 0, 1), opts(2, 6, 0, 0, 1), opts(0, 0, 2, 4, 1), opts(2, 0, 4, 16, 1), opts(0, 1, 4, 4, 0),
         opts(2, 1, 2, 16, 0), opts(0, 6, 2, 16, 1), opts(2, 6, 4, 4, 0), opts(0, 0, 4, 0, 0), opts(2, 0, 2, 0, 1),
         opts(0, 1, 0, 16, 1), opts(2, 1, 0, 4, 1), opts(0, 6, 4, 16, 0), opts(2, 0, 0, 16, 0)]
SHORT_SWEEP = [SWEEP[1], SWEEP[2], SWEEP[5], SWEEP[8]]
for _boot in (0, 2):
    for _key, _values in (("bm_round", {0, 1, 6}), ("bm_queries_per_group", {0, 2, 4}), ("bm_waves", {0, 4, 16}),
                          ("bm_runs", {0, 1})):
        assert {o[_key] for o in SWEEP if o["bm_boot"] == _boot} == _values, (_boot, _key)


# ------------------------------------------------------------------------------------------------ the cases --
def sparse_case(M, nq=9):
    """Case 1: 3001 uniformly drawn rows over 1024 buckets (about 3 rows each) and 65536 runs."""
    return make_case(9400 + M + nq, dims(M), [8] * M, 3001, nq, dup_frac=0.03)


SKEW_FIRST = (17, 90, 91, 203)          # the four first codes of case 2 ...
SKEW_SIZES = (1, 63, 65, 5871)          # ... and the rows carrying each: N = 6000, the last above BM_BOOT_ROWS
SKEW_SEED = 9502
SKEW_TAIL_QUERY, SKEW_EMPTY_QUERY = 3, 12


def skewed_case():
    """Case 2: the first code takes four values, in buckets of 1, 63, 65 and 5871 rows (bucket_bits 8); query q
    of the first 12 is drawn near the first centroid SKEW_FIRST[q % 4], so that its nearest bucket is that one.
    Query 3 also sits on the LAST second centroid: its nearest run is the large bucket's last one, a few dozen
    rows.  Query 12 lies between the large bucket's first centroid and its nearest neighbour among the
    centroids no row carries, a little closer to that one: the nearest bucket of all is empty."""
    M, N, nq = 16, sum(SKEW_SIZES), 13
    c = make_case(SKEW_SEED, dims(M), [8] * M, N, nq)
    rng = np.random.default_rng(SKEW_SEED + 1)
    first = np.repeat(np.array(SKEW_FIRST, np.uint16), SKEW_SIZES)
    c["codes"][:, 0] = first[rng.permutation(N)]
    L = c["L"]
    Xp = (rng.normal(size=(nq, c["D"])) * 30.0).astype(np.float32)
    for q in range(12):
        Xp[q, :L] = c["cents"][0][SKEW_FIRST[q % 4]] + rng.normal(size=L).astype(np.float32)
    Xp[SKEW_TAIL_QUERY, L:2 * L] = c["cents"][1][255]
    big = c["cents"][0][SKEW_FIRST[3]]
    away = ((c["cents"][0] - big) ** 2).sum(axis=1)
    away[list(SKEW_FIRST)] = np.inf
    Xp[SKEW_EMPTY_QUERY, :L] = 0.45 * big + 0.55 * c["cents"][0][int(np.argmin(away))]
    c["X"] = np.ascontiguousarray(Xp @ c["eig"].T, dtype=np.float32)  # (projection: X @ eig, eig orthogonal)
    return c


def nearest_run_start(lut, codes, bucket_bits):
    """bm_boot_kernel's choice restated: the non-empty bucket of the smallest key (bound bits above the index
    bits | bucket), inside it the non-empty run of the smallest second term (ties: the smaller code).  Returns
    (bucket, rows of the bucket, offset of that run's first row in the bucket)."""
    bt = bucket_bits - 8
    K0 = 256 << bt
    ids = bucket_ids(codes, bucket_bits)
    rows = np.bincount(ids, minlength=K0)
    w = 8 - bt
    gmin = lut[1].reshape(1 << bt, 1 << w).min(axis=1)
    b_all = np.arange(K0)
    bound = (lut[0][b_all >> bt] + gmin[b_all & ((1 << bt) - 1)]).astype(np.float32) if bt else lut[0][b_all]
    key = (bound.view(np.uint32).astype(np.int64) & ~np.int64(K0 - 1)) | b_all
    key[rows == 0] = np.iinfo(np.int64).max
    b = int(np.argmin(key))
    second = codes[ids == b, 1].astype(np.int64) & ((1 << w) - 1)
    present = np.unique(second)
    c1base = (b & ((1 << bt) - 1)) << w
    term = lut[1][c1base + present]
    j = int(present[np.lexsort((present, term.view(np.uint32)))[0]])
    return b, int(rows[b]), int((second < j).sum())


SMALL_N = [(1, 8, 8), (7, 16, 8), (40, 32, 8), (300, 16, 10)]  # N, M, bucket_bits
SMALL_K = {1: (100, 256), 7: (100, 256), 40: (100, 256), 300: (256,)}


def small_case(N, M):
    """Case 3: fewer rows than k (and, with 300 rows, barely more)."""
    return make_case(9600 + N, dims(M), [8] * M, N, 5, dup_frac=0.1)


NONFINITE_FIRST, NONFINITE_SECOND = 77, 140  # the centroids at 3e38 in the first and in the second subspace
NONFINITE_K = (10, 100, 256)


def nonfinite_case():
    """Case 6: no rotation; one centroid of the first and one of the second subspace lie at 3e38, so their table
    entries are +inf for every query; most rows carry one of them and fewer than 256 rows stay finite.  Query 1
    is all NaN, query 2 has one +inf coordinate in the first subspace, query 3 one in the third."""
    M, N, nq = 8, 3001, 7
    c = make_case(9700, dims(M), [8] * M, N, nq, dup_frac=0.03, rotate=False)
    rng = np.random.default_rng(9701)
    c["cents"][0][NONFINITE_FIRST] = 3e38
    c["cents"][1][NONFINITE_SECOND] = 3e38
    codes = c["codes"]
    for s, bad in ((0, NONFINITE_FIRST), (1, NONFINITE_SECOND)):  # the uniform draw's few: moved off first
        hit = codes[:, s] == bad
        codes[hit, s] = (bad + 1 + rng.integers(0, 254, int(hit.sum()))) % 256
    rows = rng.permutation(N)
    codes[rows[:1400], 0] = NONFINITE_FIRST
    codes[rows[1400:2800], 1] = NONFINITE_SECOND
    codes[rows[2800:2810], 0] = NONFINITE_FIRST   # ... and a few carry both
    codes[rows[2800:2810], 1] = NONFINITE_SECOND
    c["X"][1] = np.nan
    c["X"][2, 5] = np.inf
    c["X"][3, 2 * c["L"] + 1] = np.inf
    return c


TIED_BLOCK, TIED_N, TIED_DISTINCT = 5000, 6000, 12
TIED_K = (10, 256)


def tied_case():
    """Case 7: small-integer centroids; 5000 of the 6000 rows are one code vector, the others are copies of 12
    more, all scattered over the labels: every distance occurs dozens of times, one of them 5000 times."""
    M, nq = 8, 12
    c = make_case(9801, dims(M), [8] * M, TIED_N, nq, integer=True)
    rng = np.random.default_rng(9802)
    vecs = c["codes"][: TIED_DISTINCT + 1].copy()
    which = np.concatenate([np.zeros(TIED_BLOCK, np.int64), 1 + rng.integers(0, TIED_DISTINCT, TIED_N - TIED_BLOCK)])
    c["codes"] = np.ascontiguousarray(vecs[which[rng.permutation(TIED_N)]])
    return c


def growth_case():
    """Case 9: a sparse index with 33 queries, and 64 more rows that all fall into one bucket (bucket_bits 10)
    that was empty before."""
    c = sparse_case(16, nq=33)
    rng = np.random.default_rng(9901)
    occupied = np.bincount(bucket_ids(c["codes"], 10), minlength=1024)
    b = int(np.nonzero(occupied == 0)[0][3])
    more = rng.integers(0, 256, size=(64, 16)).astype(np.uint16)
    more[:, 0] = b >> 2
    more[:, 1] = ((b & 3) << 6) | rng.integers(0, 64, 64)
    return c, more, b


# -------------------------------------------------------------------------------------------------- checking --
def expect(oracle, c, X, k, id_base=0, codes=None):
    """What the oracle says of queries X: labels (moved by id_base), distances, all distances."""
    c = c if codes is None else dict(c, codes=codes)
    Xp = oracle.project(X, c["eig"]) if c["eig"] is not None else X
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True)
    o_lab = np.where(o_lab >= 0, o_lab + id_base, -1).astype(np.int32)
    return o_lab, o_dis, oracle_all_dists(oracle, c, Xp)


def check_rounds(v, X, k, want, sweep, id_base=0, what="", bm=1):
    """bucket_major = 0 against the oracle; then every entry of the sweep under bucket_major = 2 against the
    oracle and bit for bit against that first answer.  (An answer that equals the first one bit for bit meets
    the tie contract because that one did; one that differs goes through the contract's own check first, which
    says how it differs from the oracle.)  Returns the last timing."""
    o_lab, o_dis, ad = want
    base_l, base_d, t0 = run(v, X, k, bucket_major=0)
    assert t0["bucket_major"] == 0, what
    assert_topk_matches(base_l, base_d, o_lab, o_dis, ad, id_base=id_base, what=f"{what} one workgroup per query")
    t = t0
    for o in sweep:
        l, d, t = run(v, X, k, bucket_major=2, **o)
        w = f"{what} k={k} {o}"
        assert t["bucket_major"] == bm, w
        assert np.array_equal(d.view(np.uint32), o_dis.view(np.uint32)), w
        same = np.array_equal(d.view(np.uint32), base_d.view(np.uint32)) and np.array_equal(l, base_l)
        if not same:
            assert_topk_matches(l, d, o_lab, o_dis, ad, id_base=id_base, what=w)
        assert same, w
    return t


def timed_index(c, bucket_bits, sub_order=1, id_base=0):
    import vaq_amd
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(c["bits"])
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v._ensure_index()
    v.set_option("sub_order", sub_order)
    v.set_option("bucket_bits", bucket_bits)
    v.id_base = id_base
    v.mCodebook = c["codes"]
    v.set_option("timing", 1)
    return v


_REF = {}


def sparse_reference(oracle, M):
    """Case 1's index data and the oracle's answers for every k, computed once and shared (never written to)."""
    if M not in _REF:
        c = sparse_case(M)
        _REF[M] = (c, {k: expect(oracle, c, c["X"], k) for k in (1, 10, 100, 256, 257)})
    return _REF[M]


# ----------------------------------------------------------------------------------------------------- tests --
@pytest.mark.parametrize("M", [8, 16, 32])
def test_sparse_buckets(vaqlib, oracle, M):
    """Case 1: about 3 rows per bucket -- empty buckets (the be > bs tests of mark and boot), buckets of one row,
    partly filled waves, nearly every run empty, an order kernel with most buckets at zero work.  Rows ordered
    inside the buckets and not (sub_order)."""
    c, want = sparse_reference(oracle, M)
    for sub_order in (1, 0):
        v = timed_index(c, 10, sub_order)
        for k in (1, 10, 100, 256):
            check_rounds(v, c["X"], k, want[k], SWEEP if sub_order else SHORT_SWEEP, what=f"sparse M={M} sub_order={sub_order}")
        v.close()


@pytest.mark.parametrize("bucket_bits", [8, 9])
def test_skewed_buckets_and_boot_clipping(vaqlib, oracle, bucket_bits):
    """Case 2: buckets of 1, 63, 65 and 5871 rows among 252 empty ones, every query aimed at one of them: the
    sample behind a sampled threshold has fewer rows than k (the threshold stays FLT_MAX), between k and 4096,
    and is clipped at 4096 -- from the nearest run on, or, where that run starts in the bucket's last 4096
    rows, the 4096 rows before the bucket's end.  bucket_bits 9 halves the buckets over the same codes (a
    shorter sweep)."""
    c = skewed_case()
    v = timed_index(c, bucket_bits)
    for k in (10, 100):
        check_rounds(v, c["X"], k, expect(oracle, c, c["X"], k), SWEEP if bucket_bits == 8 else SHORT_SWEEP,
                     what=f"skewed bucket_bits={bucket_bits}")
    v.close()


def test_short_tail_sample_keeps_the_candidate_buffer(vaqlib, oracle):
    """Case 2, the query whose nearest run is the large bucket's last few dozen rows, k = 100, 256 candidate
    slots.  The sample is the bucket's last 4096 rows, so fewer than 256 rows of the whole index lie at or
    below its k-th distance (the CPU companion counts them with the oracle): no buffer overflows and no query
    is left to the best-first form.  (Results cannot tell which rows were sampled -- any sample's k-th distance is a
    valid bound, and a buffer that overflows under a loose one is retried -- so this bound on the count is the
    only thing pinned here about the short tail; the answers are checked as everywhere.)"""
    c = skewed_case()
    X, k = c["X"][SKEW_TAIL_QUERY:SKEW_TAIL_QUERY + 1], 100
    want = expect(oracle, c, X, k)
    v = timed_index(c, 8)
    for rnd in (0, 1, 6):
        t = check_rounds(v, X, k, want, [opts(2, rnd, 0, 0, 1, cap=256)], what="short tail")
        assert t["deferred_queries"] == 0, (rnd, t)
    v.close()


def test_first_round_thresholds(vaqlib, oracle):
    """Case 2, staged, a sampled threshold and no middle round: the first half is the sample and the round of
    every query's nearest NON-EMPTY bucket.  The threshold it hands out is then the k-th smallest distance
    inside that bucket (the oracle's), or FLT_MAX where the bucket has fewer than k rows -- for query 12 too,
    whose nearest bucket of all is empty and must not be the one the round spends itself on."""
    import torch
    c = skewed_case()
    nq, k = c["X"].shape[0], 10
    o_lab, o_dis, ad = expect(oracle, c, c["X"], k)
    Xp = oracle.project(c["X"], c["eig"])
    ids = bucket_ids(c["codes"], 8)
    thr_want = np.empty(nq, np.float32)
    for q in range(nq):
        b, n, _ = nearest_run_start(oracle.create_lut(Xp[q], c["cents"], 8), c["codes"], 8)
        thr_want[q] = np.sort(ad[q][ids == b])[k - 1] if n >= k else FLT_MAX
    assert (thr_want == FLT_MAX).sum() == 3 and thr_want[SKEW_EMPTY_QUERY] < FLT_MAX
    v = timed_index(c, 8)
    for o in (opts(2, 0, 0, 0, 1), opts(2, 0, 2, 4, 0)):
        l, d, t = run(v, c["X"], k, bucket_major=2, **o)
        assert t["bucket_major"] == 1
        assert_topk_matches(l, d, o_lab, o_dis, ad, what="first round")
        labels = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
        dists = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
        thr = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        v.search_begin_device(torch.from_numpy(c["X"]).cuda(), k, (labels, dists), thr)
        got = thr.cpu().numpy().view(np.uint32)
        v.search_finish_device(None)
        torch.cuda.synchronize()
        assert np.array_equal(got, thr_want.view(np.uint32)), (o, got.view(np.float32), thr_want)
        assert np.array_equal(labels.cpu().numpy(), l) and np.array_equal(dists.cpu().numpy().view(np.uint32), d.view(np.uint32))
    v.close()


@pytest.mark.parametrize("N,M,bucket_bits", SMALL_N, ids=[f"n{n}_m{m}_b{b}" for n, m, b in SMALL_N])
def test_fewer_rows_than_k(vaqlib, oracle, N, M, bucket_bits):
    """Case 3: N < k -- every row comes back, in order, and the tail is -1 / FLT_MAX; and 300 rows over 1024
    buckets with k = 256, where all but 44 rows are wanted."""
    c = small_case(N, M)
    v = timed_index(c, bucket_bits)
    nq = c["X"].shape[0]
    for k in SMALL_K[N]:
        assert N < k or N == 300
        want = expect(oracle, c, c["X"], k)
        check_rounds(v, c["X"], k, want, SWEEP, what=f"N={N}")
        l, d, t = run(v, c["X"], k, bucket_major=2, **SWEEP[1])
        assert t["bucket_major"] == 1
        assert np.all(l[:, N:] == -1) and np.all(d[:, N:] == FLT_MAX)
        if N < k:
            assert np.array_equal(np.sort(l[:, :N], axis=1), np.tile(np.arange(N, dtype=np.int32), (nq, 1)))
        else:
            assert np.all(l >= 0)
    v.close()


@pytest.mark.parametrize("nq", [1, 3, 5, 8])
def test_query_count_edges(vaqlib, oracle, nq):
    """Case 4: fewer queries than a group holds, and counts that are no multiple of it."""
    c, want = sparse_reference(oracle, 16)
    v = timed_index(c, 10)
    sweep = [o for o in SWEEP if o["bm_queries_per_group"] in (2, 4)]
    assert {o["bm_queries_per_group"] for o in sweep} == {2, 4} and {o["bm_boot"] for o in sweep} == {0, 2}
    for k in (10, 100):
        check_rounds(v, c["X"][:nq], k, tuple(a[:nq] for a in want[k]), sweep, what=f"nq={nq}")
    v.close()


def test_id_base(vaqlib, oracle):
    """Case 5: labels start at 1 000 000.  After a best-first pass A select meets that pass's labelled list and
    raw candidates; after a sampled threshold only candidates."""
    base = 1_000_000
    c, _ = sparse_reference(oracle, 8)
    v = timed_index(c, 10, id_base=base)
    for k in (10, 100, 256):
        want = expect(oracle, c, c["X"], k, id_base=base)
        check_rounds(v, c["X"], k, want, SWEEP, id_base=base, what="id_base")
        for boot in (0, 2):
            l, d, t = run(v, c["X"], k, bucket_major=2, **opts(boot, 6, 0, 0, 1))
            assert t["bucket_major"] == 1
            assert np.all(l >= 0) and l.min() >= base and l.max() < base + 3001
    v.close()


@pytest.mark.parametrize("bucket_bits", [8, 10])
def test_nonfinite_tables(vaqlib, oracle, bucket_bits):
    """Case 6: bucket bounds and run terms of +inf, an all-NaN query, queries whose every distance is +inf.  A
    row with an infinite table entry is never returned; with fewer finite rows than k the tail is -1 / FLT_MAX."""
    c = nonfinite_case()
    bad = (c["codes"][:, 0] == NONFINITE_FIRST) | (c["codes"][:, 1] == NONFINITE_SECOND)
    finite = int((~bad).sum())
    v = timed_index(c, bucket_bits)
    for k in NONFINITE_K:
        want = expect(oracle, c, c["X"], k)
        check_rounds(v, c["X"], k, want, SWEEP, what=f"non-finite bucket_bits={bucket_bits}")
        l, d, t = run(v, c["X"], k, bucket_major=2, **SWEEP[3])
        assert t["bucket_major"] == 1
        assert not np.any(bad[l[l >= 0]])
        assert np.all(l[1:4] == -1) and np.all(d[1:4] == FLT_MAX)
        for q in (0, 4, 5, 6):
            assert np.all(l[q, :min(k, finite)] >= 0) and np.all(l[q, finite:] == -1) and np.all(d[q, finite:] == FLT_MAX)
    v.close()


@pytest.mark.parametrize("k", TIED_K)
def test_identical_rows_beyond_the_candidate_buffer(vaqlib, oracle, k):
    """Case 7: 5000 rows of one distance against 1, 8 and 64 candidate slots: an overflowed query keeps its place
    and is planned again under the bound "the k-th pair so far, label included"; with one slot some queries
    are still left to the best-first form.  The answers are the smallest labels of the tied distance (the
    boundary rule of assert_topk_matches, which every query of this case meets)."""
    c = tied_case()
    v = timed_index(c, 8)
    want = expect(oracle, c, c["X"], k)
    for cap in (1, 8, 64):
        sweep = [dict(o, bm_candidates=cap) for o in SWEEP]
        check_rounds(v, c["X"], k, want, sweep, what=f"tied cap={cap}")
        for boot in (0, 2):
            _, _, t = run(v, c["X"], k, bucket_major=2, **opts(boot, 6, 0, 0, 1, cap))
            assert t["bucket_major"] == 1 and t["deferred_queries"] >= 0
            if cap == 1:
                assert t["deferred_queries"] > 0, (k, boot, t)
    v.close()


def test_refusals(vaqlib, oracle):
    """Case 8: 128 buckets cut from the first code's top 7 bits (a bucket shift), 2048 and 4096 buckets, and
    k = 257 are not the rounds': the plan falls back without a word and the answer is the oracle's.  k = 256 on
    the same index takes them."""
    c, want = sparse_reference(oracle, 16)
    for bucket_bits in (7, 11, 12):
        v = timed_index(c, bucket_bits)
        for k in (10, 256):
            check_rounds(v, c["X"], k, want[k], SHORT_SWEEP, what=f"refused bucket_bits={bucket_bits}", bm=0)
        v.close()
    v = timed_index(c, 10)
    check_rounds(v, c["X"], 257, want[257], SHORT_SWEEP, what="refused k=257", bm=0)
    check_rounds(v, c["X"], 256, want[256], SHORT_SWEEP, what="k=256", bm=1)
    v.close()


def test_reuse_and_growth(vaqlib, oracle):
    """Case 9: one index serves 3 queries with k = 10, 33 with k = 100, the first again (workspaces grown, then
    larger than needed), and after 64 appended rows that fill one bucket that was empty, once more."""
    c, more, _ = growth_case()
    v = timed_index(c, 10)
    for nq, k in ((3, 10), (33, 100), (3, 10)):
        check_rounds(v, c["X"][:nq], k, expect(oracle, c, c["X"][:nq], k), SHORT_SWEEP, what=f"reuse nq={nq}")
    v.add_codes(more)
    grown = np.concatenate([c["codes"], more])
    assert v.info()["N"] == grown.shape[0]
    for nq, k in ((33, 100), (3, 10)):
        check_rounds(v, c["X"][:nq], k, expect(oracle, c, c["X"][:nq], k, codes=grown), SWEEP, what=f"grown nq={nq}")
    v.close()


def test_staged_search_small_index(vaqlib, oracle):
    """Case 10: vaqhip_search_begin_device / _finish_device(NULL) on 3001 rows give exactly what search gives.
    With a sampled threshold and no middle round the first half runs the sample's round alone; with neither
    (bm_boot 0, bm_round 0) it runs no round at all and only makes the 64-bit threshold words (r_split == 0 in
    run_bucket_major)."""
    import torch
    c, want = sparse_reference(oracle, 16)
    nq = c["X"].shape[0]
    v = timed_index(c, 10)
    Xd = torch.from_numpy(c["X"]).cuda()
    for k in (10, 256):
        o_lab, o_dis, ad = want[k]
        for boot, rnd in ((2, 0), (0, 0), (0, 6)):
            l, d, t = run(v, c["X"], k, bucket_major=2, **opts(boot, rnd, 0, 0, 1))
            assert t["bucket_major"] == 1
            assert v.staged_supported(nq, k)
            labels = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
            dists = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
            thr = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
            v.search_begin_device(Xd, k, (labels, dists), thr)
            v.search_finish_device(None)
            torch.cuda.synchronize()
            sl, sd = labels.cpu().numpy(), dists.cpu().numpy()
            w = f"staged k={k} boot={boot} round={rnd}"
            # (a threshold is an upper bound of the final k-th distance, as distance bits)
            assert np.all(thr.cpu().numpy().view(np.uint32) >= o_dis[:, k - 1].view(np.uint32)), w
            assert_topk_matches(l, d, o_lab, o_dis, ad, what=w)
            assert np.array_equal(sl, l) and np.array_equal(sd.view(np.uint32), d.view(np.uint32)), w
    v.close()
