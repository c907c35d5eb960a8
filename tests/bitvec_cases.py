"""Input builders of the Hamming engine's edge tests (tests/test_bitvec_edges_gpu.py).  Each builder asserts the
condition that makes its input worth running -- the tail bits hold noise, a run of equal distances crosses slot k,
the k-th best distance lies in a top bin, the answers on the two sides of a seam differ -- and
tests/test_bitvec_ref_cpu.py calls every builder, so the conditions are checked without a GPU.  The checker is the
restatement, tests/bitvec_ref.py; nothing here knows the device."""
from __future__ import annotations

import numpy as np

import bitvec_ref as br

QUERY_CHUNK = 16384  # queries per internal launch set (vaqhip_index.h)
RR_THREADS = 256     # threads of the rerank's workgroup (vaq_bitvec.hip): the query row is staged with this stride
REFINER_MAX_DIM = (64 * 1024 - 4 * 2048 * 4 - 64) // 4      # refine_rows_max_dim(): the widest row a VaqRefiner takes
RERANK_MAX_DIM = (64 * 1024 - 8 * 1024 - 256) // 4          # bitvec_rerank_max_dim()


def words(rs, n, W):
    """n random rows of W full 64-bit words"""
    return rs.randint(0, 1 << 32, (n, W), dtype=np.uint64) | (rs.randint(0, 1 << 32, (n, W), dtype=np.uint64) << np.uint64(32))


def near(rs, centre, n, flip):
    """n rows around one centre row with `flip` random bits turned: small distances with many ties"""
    W = centre.shape[0]
    rows = np.repeat(centre[None, :], n, axis=0).copy()
    for r in range(n):
        for b in rs.randint(0, 64 * W, flip):
            rows[r, b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return rows


def select_m(W):
    """bitvec_select_m (vaq_bitvec.h): the selection's histogram has 255 M + 1 bins"""
    return (64 * W + 254) // 255


def crosses(d, k):
    """a run of equal values crosses slot k of the sorted d"""
    s = np.sort(d)
    return len(s) > k and s[k - 1] == s[k]


# ---- A. every width -------------------------------------------------------------------------------------------------

def every_width(W, n=1025, nq=65, k=17):
    """(n_bits, rows, queries) for one scan kernel: two row tiles + 1 row, a query tile + 1; 64 W - 13 bits where W is
    odd (13 tail bits of noise), full words where it is even; half the rows around query 0."""
    rs = np.random.RandomState(1000 + W)
    n_bits = 64 * W - 13 if W % 2 else 64 * W
    rows = words(rs, n, W)
    rows[::2] = near(rs, rows[0], (n + 1) // 2, 6)
    queries = words(rs, nq, W)
    queries[0] = rows[0]
    if n_bits % 64:
        tail = np.uint64((1 << (64 - n_bits % 64)) - 1)
        assert (rows[:, -1] & tail).any() and (queries[:, -1] & tail).any(), "the tail bits hold nothing"
    d0 = br.hamming_dists(rows, queries[:1])[0]
    assert crosses(d0, k) and len(np.unique(d0[:k])) < k, "query 0 has no crowd of ties at its head"
    return n_bits, rows, queries


# ---- B. the far crowd -----------------------------------------------------------------------------------------------

FAR_WIDTHS = (1, 3, 4, 8, 12, 16)  # 4, 8, 12, 16: 64 W is the first past a multiple of 255, where M steps; 1, 3: controls


def far_crowd(W, n=600, seed=0):
    """(rows, queries): rows are the complement of query 0 with 0..3 distinct bits turned back, so every distance of
    query 0 is one of 64 W - 3 .. 64 W, about n / 4 rows on each; query 1 is random."""
    rs = np.random.RandomState(2000 + 16 * seed + W)
    queries = words(rs, 2, W)
    rows = np.repeat(~queries[:1], n, axis=0)
    flips = rs.randint(0, 4, n)
    for r in range(n):
        for b in rs.choice(64 * W, flips[r], replace=False):
            rows[r, b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    d0 = br.hamming_dists(rows, queries[:1])[0]
    assert np.array_equal(d0, 64 * W - flips)
    assert all((d0 == 64 * W - f).sum() >= 8 for f in range(4)), "a distance of the top four is (nearly) absent"
    return rows, queries


def far_k(rows, queries, off):
    """the k at which the k-th best distance of query 0 is 64 W - off and slot k lies in the middle of its run"""
    W = rows.shape[1]
    d0 = br.hamming_dists(rows, queries[:1])[0]
    want = 64 * W - off
    k = int((d0 < want).sum() + (d0 == want).sum() // 2)
    check_far(rows, queries, k, off)
    return k


def check_far(rows, queries, k, off):
    """the k-th best distance of query 0 is 64 W - off, and its run of equal distances crosses slot k"""
    W = rows.shape[1]
    s = np.sort(br.hamming_dists(rows, queries[:1])[0])
    assert 1 <= k <= 1024 and k < len(s)
    assert s[k - 1] == 64 * W - off and s[k] == s[k - 1], (W, k, off)
    assert 255 * select_m(W) >= 64 * W  # the distance has a bin of its own


# ---- C. chunk seams -------------------------------------------------------------------------------------------------

PERIOD = 7  # does not divide QUERY_CHUNK: the residue of the first query behind a seam is not 0


def periodic(base, nq):
    """query i = base[i % PERIOD]"""
    assert base.shape[0] == PERIOD and QUERY_CHUNK % PERIOD
    return np.ascontiguousarray(base[np.arange(nq) % PERIOD])


def seam_window(nq):
    """the first period and the ten queries around the seam at QUERY_CHUNK"""
    assert nq >= QUERY_CHUNK + 5
    return np.concatenate([np.arange(PERIOD), np.arange(QUERY_CHUNK - 5, QUERY_CHUNK + 5)])


def distinct_answers(lab, dis):
    rows = {(tuple(l), tuple(d)) for l, d in zip(lab.tolist(), dis.tolist())}
    return len(rows) == len(lab)


def seam_query(n=64, k=3):
    """(rows, base queries, the restatement's answers of the base queries): W = 1.  A query answered from another
    query's offset is seen only if the answers differ, so the seven are pairwise different."""
    rs = np.random.RandomState(31)
    rows = words(rs, n, 1)
    base = near(rs, rows[5], PERIOD, 9)
    want = br.query_sort(rows, base, k)
    assert distinct_answers(*want), "two residues share an answer"
    return rows, base, want


def seam_rerank(n=64, k=2, factor=2, D=4):
    """(rows, base bit queries, X uint8, base raw queries, the restatement's answers): the bit queries and the raw
    queries repeat together.  The bit queries, the raw queries and the answers are each pairwise different, so any
    one of the three offsets (d_bq, d_oq, d_labels) gone wrong changes an answer."""
    rs = np.random.RandomState(32)
    rows = words(rs, n, 1)
    base = near(rs, rows[9], PERIOD, 9)
    X = rs.randint(0, 256, (n, D)).astype(np.uint8)
    XQ = rs.randint(0, 256, (PERIOD, D)).astype(np.float32)
    want = br.query_rerank(rows, base, X, XQ, k, factor)
    assert distinct_answers(*want), "two residues share an answer"
    assert len({tuple(b) for b in base.tolist()}) == PERIOD and len({tuple(x) for x in XQ.tolist()}) == PERIOD
    # the raw query decides: with the raw queries of the next residue the answers change
    other = br.query_rerank(rows, base, X, np.roll(XQ, 1, axis=0), k, factor)
    assert all(not np.array_equal(a, b) for a, b in zip(want[1], other[1]))
    return rows, base, X, XQ, want


def small_chunks(n=100, W=3, nq=5, D=7):
    """(rows, queries, X uint8, XQ) for the runs under a small dist_chunk_bytes: five queries whose answers differ"""
    rs = np.random.RandomState(33)
    rows = near(rs, words(rs, 1, W)[0], n, 12)
    queries = near(rs, rows[0], nq, 8)
    X = rs.randint(0, 4, (n, D)).astype(np.uint8)
    XQ = rs.randint(0, 4, (nq, D)).astype(np.float32)
    assert distinct_answers(*br.query_sort(rows, queries, 17))
    assert distinct_answers(*br.query_rerank(rows, queries, X, XQ, 5, 3))
    return rows, queries, X, XQ


# ---- D. rerank launch edges -----------------------------------------------------------------------------------------

# past RR_THREADS (the staging loop's second step) with D % 4 = 1, 2, 0; four steps; the widest row a refiner holds
RERANK_DIMS = (257, 258, 260, 1024, REFINER_MAX_DIM)


def rerank_edge(D, n=40, nq=3, k=5, factor=4):
    """(rows, queries, Xf, XQf, Xb, XQb): bit rows of two words; general float rows; byte rows that differ from one
    base row in four columns each, anywhere in the row, so their distances are small integers with ties inside the
    head and across slot k."""
    rs = np.random.RandomState(4000 + D)
    rows = near(rs, words(rs, 1, 2)[0], n, 9)
    queries = near(rs, rows[0], nq, 5)
    Xf = rs.standard_normal((n, D)).astype(np.float32) * np.float32(37.5)
    XQf = rs.standard_normal((nq, D)).astype(np.float32) * np.float32(37.5)
    base = rs.randint(0, 4, D).astype(np.uint8)
    Xb = np.repeat(base[None, :], n, axis=0)
    XQb = np.repeat(base[None, :].astype(np.float32), nq, axis=0)
    for r in range(n):
        Xb[r, rs.choice(D, 4, replace=False)] += np.uint8(1)
        if r % 2:
            Xb[r, D - 1 - r % 3] += np.uint8(1)  # (the last columns, which the scalar remainder loop reads)
    for q in range(nq):
        XQb[q, rs.choice(D, 2, replace=False)] += np.float32(1)
    # some row differs from the base behind the first RR_THREADS columns
    assert D > RR_THREADS and (Xb[:, RR_THREADS:] != base[RR_THREADS:]).any()
    cand, _ = br.query_sort(rows, queries, min(factor * k, n))
    inside = across = False
    for q in range(nq):
        e = br.euclidean_no_sqrt(XQb[q], Xb[cand[q]])
        inside |= len(np.unique(e[:k])) < k
        across |= bool(crosses(e, k))
    assert inside and across, "the byte rows have no equal distances inside the head and across slot k"
    return rows, queries, Xf, XQf, Xb, XQb


# ---- E. infinite distances ------------------------------------------------------------------------------------------

def infinite_case(n=48, nq=3, k=40, factor=2, D=4):
    """(rows, queries, X, XQ, k, factor): every third row sits at +-3e19 in one coordinate, so its squared distance,
    9e38, is past FLT_MAX: +inf from finite inputs.  factor * k > n, so all n rows are candidates: 32 finite ones,
    then 16 infinite ones in candidate order, and slot k = 40 falls inside that run -- some of the infinite
    candidates lie in the head std::sort walks (the first k), the others behind it."""
    rs = np.random.RandomState(51)
    rows = near(rs, words(rs, 1, 2)[0], n, 9)
    queries = near(rs, rows[0], nq, 5)
    X = rs.standard_normal((n, D)).astype(np.float32) * np.float32(37.5)
    for r in range(0, n, 3):
        X[r, r % D] = np.float32(3e19) * (1 if r % 2 else -1)
    XQ = rs.standard_normal((nq, D)).astype(np.float32) * np.float32(37.5)
    assert np.isfinite(X).all() and np.isfinite(XQ).all()
    with np.errstate(over="ignore"):
        cand, _ = br.query_sort(rows, queries, min(factor * k, n))
        for q in range(nq):
            e = br.euclidean_no_sqrt(XQ[q], X[cand[q]])
            assert not np.isnan(e).any()
            n_inf = int(np.isinf(e).sum())
            assert n_inf * 3 == len(e), "a third of the candidates are infinitely far"
            assert len(e) - n_inf < k < len(e), "slot k is not inside the run of infinities"
            assert np.isinf(e[:k]).any() and np.isinf(e[k:]).any(), "infinities on one side of the head only"
    return rows, queries, X, XQ, k, factor
