"""Input builders of the cluster form's edge tests (tests/test_bitvec_clusters_edges_gpu.py), laid out as
tests/bitvec_cases.py is for the plain query.  Each builder asserts the condition that makes its input worth running
-- the cut falls in a far bin and inside a run of equal distances that spans clusters and tiles, the centre distances
tie (or are infinite, or NaN) where the plan's fallback is meant to run, a fused sum would visit other clusters, the
answers on the two sides of a seam differ -- and tests/test_bitvec_clusters_cpu.py calls every builder, so the
conditions are checked without a GPU.  The checker is the restatement, tests/bitvec_clusters_ref.py; nothing here knows
the device."""
from __future__ import annotations

import numpy as np

import bitvec_clusters_ref as cr
import bitvec_ref as br
from bitvec_cases import PERIOD, QUERY_CHUNK, crosses, distinct_answers, far_crowd, near, words

CL_THREADS = 256            # threads of the plan's and the select's workgroup, positions of a walk tile
CLUSTERS_MAX = 4096         # BITVEC_CLUSTERS_MAX
CLUSTERS_MAX_DIM = 8176     # BITVEC_CLUSTERS_MAX_DIM
PER_QUERY_BYTES = lambda T: 4 * T + 16  # noqa: E731  what "dist_chunk_bytes" counts per query (include/vaqhip.h)


def crowd(rs, n, W, nq):
    """(rows, queries): every row and query is one base row with bits turned in six fixed positions at most"""
    base = words(rs, 1, W)[0]
    spots = rs.choice(64 * W, 6, replace=False)

    def make(m):
        out = np.repeat(base[None, :], m, axis=0)
        for r in range(m):
            for b in spots[rs.randint(0, 2, 6) == 1]:
                out[r, b // 64] ^= np.uint64(1) << np.uint64(b % 64)
        return out
    return make(n), make(nq)


def sizes_to_idx(rs, sizes):
    """a cluster index per row with the given cluster sizes, the rows of a cluster scattered"""
    return rs.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def view(rows, queries, cen, idx, oq, q, k, atleast):
    """(cand, d, clu): the candidates of query q in visiting order, their Hamming distances and their clusters"""
    cand = cr.candidates(cen, idx, oq[q], k, atleast)
    return cand, br.hamming_dists(rows[cand], queries[q:q + 1])[0], np.asarray(idx)[cand]


def tiles(cand_clusters, at):
    """the tiles of CL_THREADS positions the walk takes the candidates `at` in: a tile never spans two clusters"""
    starts = np.flatnonzero(np.r_[True, cand_clusters[1:] != cand_clusters[:-1]])
    first = starts[np.searchsorted(starts, at, side="right") - 1]  # where the candidate's cluster begins
    return {(int(f), int((p - f) // CL_THREADS)) for f, p in zip(first, at)}


def run_at_cut(d, clu, k):
    """what a case wants of the run of equal distances at the cut, from one candidate list: the value at slot k, and
    whether the run crosses slot k of the sorted list, has members among the first k candidates and behind them, and
    spans two clusters and two walk tiles"""
    s = np.sort(d)
    t = int(s[k - 1])
    at = np.flatnonzero(d == t)
    return t, dict(crosses=bool(len(s) > k and s[k] == t), before=bool((at < k).any()), behind=bool((at >= k).any()),
                   clusters=len(set(clu[at].tolist())), tiles=len(tiles(clu, at)))


# ---- A. every width -------------------------------------------------------------------------------------------------

# the walk's tile loop ends exactly on a tile (256), one short of it (255), one past it (257), after three tiles (513);
# an empty cluster and one of a single row
SIZES_A = [256, 0, 513, 1, 255, 257]
K_A, ATLEAST_A, ID_BASE_A = 17, 3, 1000


def every_width(W, nq=9):
    """(n_bits, rows, queries, centres, clust_idx, raw queries) for cluster_select_kernel<W>: half the rows random (their
    distances spread round 32 W), half around query 0; 64 W - 13 bits where W is odd, with noise in the tail.  The
    first seed whose run of equal distances at slot k is as wanted is taken."""
    n = sum(SIZES_A)
    n_bits = 64 * W - 13 if W % 2 else 64 * W
    for seed in range(40):
        rs = np.random.RandomState(5000 + 100 * seed + W)
        rows = words(rs, n, W)
        rows[::2] = near(rs, rows[0], (n + 1) // 2, 6)
        queries = words(rs, nq, W)
        queries[0] = rows[0]
        idx = sizes_to_idx(rs, SIZES_A)
        cen = rs.standard_normal((len(SIZES_A), 5)).astype(np.float32)
        oq = rs.standard_normal((nq, 5)).astype(np.float32)
        cand, d, clu = view(rows, queries, cen, idx, oq, 0, K_A, ATLEAST_A)
        t, run = run_at_cut(d, clu, K_A)
        if run["crosses"] and run["before"] and run["behind"] and run["clusters"] >= 2:
            break
    # a run of equal distances crosses slot k, with members among the first k candidates, behind them, in two clusters
    assert run["crosses"] and run["before"] and run["behind"] and run["clusters"] >= 2, (W, t, run)
    if n_bits % 64:
        tail = np.uint64((1 << (64 - n_bits % 64)) - 1)
        assert (rows[:, -1] & tail).any() and (queries[:, -1] & tail).any(), "the tail bits hold nothing"
    assert sorted(np.bincount(idx, minlength=len(SIZES_A)).tolist()) == sorted(SIZES_A)
    assert len(cr.visited(cen, idx, oq[0], K_A, ATLEAST_A)) >= 3
    # the random half reaches the other queries at distances far from 0: cuts in other threads' bins
    assert br.hamming_dists(rows, queries[1:2])[0].min() > 8
    return n_bits, rows, queries, cen, idx, oq


# ---- B. far bins and the middle of the scan -------------------------------------------------------------------------

SIZES_B = [260, 230, 50, 40, 20]  # 600 rows in visiting order: one cluster past a tile of 256
ID_BASE_B = 3


def select_per(W):
    """PER of cluster_select_kernel<W>: the bins a thread owns in the cut search"""
    return (64 * W + 1 + CL_THREADS - 1) // CL_THREADS


def far_clusters(W):
    """(rows, queries, centres, clust_idx, raw queries): bc.far_crowd(W) over five clusters.  The centres lie on a line
    and both raw queries near its start, so both visit the clusters in the order 0, 1, 2, 3, 4."""
    rows, queries = far_crowd(W)
    rs = np.random.RandomState(6000 + W)
    idx = sizes_to_idx(rs, SIZES_B)
    T = len(SIZES_B)
    cen = np.zeros((T, 3), np.float32)
    cen[:, 0] = np.arange(1, T + 1)
    cen[:, 1:] = rs.standard_normal((T, 2)).astype(np.float32) * np.float32(0.01)
    oq = np.array([[0.0, 0.25, -0.5], [-0.125, 0.0, 0.375]], np.float32)
    for q in range(2):
        assert np.array_equal(cr.centre_order(cen, oq[q]), np.arange(T))
    return rows, queries, cen, idx, oq


def far_k(case, off, atleast):
    """the k at which query 0's cut is 64 W - off with slot k in the middle of the run there, worked out over the
    candidates in visiting order; moved by a few where query 1 has no run across slot k.  With atleast = 1 the
    candidates depend on k: the clusters walked are tried from one upwards until k is consistent with them."""
    rows, queries, cen, idx, oq = case
    W, T = rows.shape[1], len(cen)
    want = 64 * W - off
    sizes = np.bincount(idx, minlength=T)
    for walked in ([T] if atleast == T else range(1, T)):
        cand = np.concatenate([np.flatnonzero(idx == c) for c in range(walked)])
        d0 = br.hamming_dists(rows[cand], queries[:1])[0]
        mid = int((d0 < want).sum() + (d0 == want).sum() // 2)
        for k in (mid + s * m for m in range(9) for s in (1, -1)):
            if not 1 <= k <= 1024 or (atleast == 1 and not sizes[:walked - 1].sum() < k <= sizes[:walked].sum()):
                continue
            if problems_far(case, k, off, atleast) == []:
                return k
    raise AssertionError((W, off, atleast, "no k puts the cut there"))


def problems_far(case, k, off, atleast):
    """what check_far would object to, as a list (empty: nothing)"""
    rows, queries, cen, idx, oq = case
    W, T = rows.shape[1], len(cen)
    out = []
    walk = cr.visited(cen, idx, oq[0], k, atleast)
    if not np.array_equal(walk, cr.visited(cen, idx, oq[1], k, atleast)):
        out.append("the two queries walk other clusters")
    if (len(walk) == T) != (atleast == T):
        out.append("the clusters walked are not all / not a strict subset")
    cand, d, clu = view(rows, queries, cen, idx, oq, 0, k, atleast)
    t, run = run_at_cut(d, clu, k)
    if t != 64 * W - off:
        out.append("query 0's cut is %d" % t)
    if not (run["crosses"] and run["before"] and run["behind"]):
        out.append("slot k is not inside the run, with members before and behind position k")
    if run["clusters"] < 2 or run["tiles"] < 2:
        out.append("the run lies in one cluster or one tile")
    cand, d, clu = view(rows, queries, cen, idx, oq, 1, k, atleast)
    if not crosses(d, k):
        out.append("query 1 has no run across slot k")
    return out


def check_far(case, k, off, atleast):
    """query 0's cut is 64 W - off: slot k lies inside the run there, which has members among the first k candidates
    and behind them, in two clusters and two tiles at least; query 1 has a run of equal distances across slot k, with
    its cut in a middle thread's bins; atleast = T walks every cluster, atleast = 1 a strict subset"""
    assert problems_far(case, k, off, atleast) == [], (k, off, atleast)
    rows, queries, cen, idx, oq = case
    W = rows.shape[1]
    cand, d, clu = view(rows, queries, cen, idx, oq, 1, k, atleast)
    t1 = int(np.sort(d)[k - 1])
    assert 16 * W <= t1 <= 48 * W, (W, t1)
    per = select_per(W)
    assert (64 * W) // per > t1 // per > 0  # bin b belongs to thread b // PER: three different owners (0, t1's, 64 W's)


FULL_HEAD = dict(W=8, n=1100, k=1024, sizes=[400, 300, 250, 150])


def full_head():
    """(rows, queries, centres, clust_idx, raw queries, k): k = 1024 of 1100 rows, every cluster walked: inv[], keys[]
    and the bitonic sort at their full size, query 0's cut at 64 W"""
    W, n, k, sizes = FULL_HEAD["W"], FULL_HEAD["n"], FULL_HEAD["k"], FULL_HEAD["sizes"]
    rows, queries = far_crowd(W, n=n)
    rs = np.random.RandomState(6100)
    idx = sizes_to_idx(rs, sizes)
    cen = rs.standard_normal((len(sizes), 3)).astype(np.float32)
    oq = rs.standard_normal((2, 3)).astype(np.float32)
    cand, d, clu = view(rows, queries, cen, idx, oq, 0, k, len(sizes))
    t, run = run_at_cut(d, clu, k)
    assert len(cand) == n and t == 64 * W and run["crosses"] and run["before"] and run["behind"] and run["clusters"] >= 2
    return rows, queries, cen, idx, oq, k


# ---- C. plan edges --------------------------------------------------------------------------------------------------

K_C = 17
# (T, D, nq): the per-thread stride edge; the limit of T (16 centres a thread, a one-thread std::sort of 4096 pairs in
# the fallback: few queries); the limits of D (the query row sizes the first LDS region at 8176: 32704 bytes beside 72
# of pairs); 4 D < 8 T, and the two nearly equal from either side (796 < 800 < 804)
PLAN_SHAPES = [(255, 4, 5), (256, 4, 5), (257, 4, 5), (4095, 4, 3), (4096, 4, 3), (9, 1, 5), (9, 8176, 3), (300, 4, 5),
               (100, 199, 4), (100, 201, 4)]
PLAN_TIE_SHAPES = [s for s in PLAN_SHAPES if s[1] == 4 and s[0] != 300]


def bit_rows_c(rs, nq, n=900):
    return crowd(rs, n, 2, nq)


def dists_of(cen, oq):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([br.euclidean_no_sqrt(q, cen) for q in oq])


def empty_the_nearest(idx, cen, oq0, rs, which=(1, 2, 4)):
    """the rows of query 0's second, third and fifth nearest clusters moved to other clusters"""
    order = cr.centre_order(cen, oq0)
    T = len(cen)
    gone = [int(order[w]) for w in which if w < T - 1]
    keep = np.setdiff1d(np.arange(T), gone)
    idx = idx.copy()
    move = np.isin(idx, gone)
    idx[move] = keep[rs.randint(0, len(keep), int(move.sum()))]
    return idx, gone


def plan_shape(T, D, nq, ties):
    """(rows, queries, centres, clust_idx, raw queries, atleast): T centres of D floats, the rows assigned at random,
    several of the clusters nearest to query 0 empty.  ties: duplicated centres and pairs mirrored about query 0, as
    test_centre_order makes them (the fallback runs for query 0); else every distance of every query distinct."""
    rs = np.random.RandomState(7000 + 3 * T + D + (50000 if ties else 0))
    cen = rs.standard_normal((T, D)).astype(np.float32)
    oq = rs.standard_normal((nq, D)).astype(np.float32)
    if ties:
        oq[0] = 0
        cen[1::4] = cen[0::4][:len(cen[1::4])]    # duplicates
        m = len(cen[3::4])
        cen[2::4][:m] = -cen[3::4]                # mirrored about the origin, query 0
    else:
        for q in range(nq):  # (4096 float distances do collide now and then: draw that query again)
            while len(np.unique(br.euclidean_no_sqrt(oq[q], cen))) < T:
                oq[q] = rs.standard_normal(D).astype(np.float32)
    d = dists_of(cen, oq)
    assert np.isfinite(d).all()
    if ties:
        assert len(np.unique(d[0])) < T // 2 + 2
    else:
        assert all(len(np.unique(d[q])) == T for q in range(nq))
    rows, queries = bit_rows_c(rs, nq)
    idx = rs.randint(0, T, rows.shape[0]).astype(np.int32)
    if not ties:
        idx, gone = empty_the_nearest(idx, cen, oq[0], rs)
    atleast = min(T, 5)
    walk = cr.visited(cen, idx, oq[0], K_C, atleast)
    sizes = np.bincount(idx, minlength=T)
    if not ties and T > 9:  # the walk passes over empty clusters and goes on until the members number k
        assert (sizes[walk[:-1]] == 0).sum() >= 2 and sizes[walk].sum() >= K_C, (T, D)
    if D == CLUSTERS_MAX_DIM:
        assert 4 * D == 32704 and 4 * D > 8 * T
    return rows, queries, cen, idx, oq, atleast


def fused_sums(q, X):
    """(acc, sure): euclidean_no_sqrt of every row of X as a compiler that contracts would compute it -- t = a - b
    rounded, then acc = fma(t, t, acc), one rounding for the product and the sum -- and whether that value is beyond
    doubt.  The float64 product of two float32 is exact, the float64 sum may round once more: a row whose sum lands
    within that rounding of the midpoint of two float32 is not sure."""
    q = np.asarray(q, np.float32)
    X = np.asarray(X, np.float32)
    acc = np.zeros(X.shape[0], np.float32)
    sure = np.ones(X.shape[0], bool)
    for i in range(q.shape[0]):
        t = (q[i] - X[:, i]).astype(np.float32).astype(np.float64)
        s = t * t + acc.astype(np.float64)
        acc = s.astype(np.float32)
        for side in (np.float32(np.inf), np.float32(-np.inf)):
            mid = (acc.astype(np.float64) + np.nextafter(acc, side).astype(np.float64)) / 2
            sure &= np.abs(s - mid) > np.abs(s) * 2.0 ** -49
    return acc, sure


def euclidean_fused(q, X):
    """fused_sums as a `dist` of tests/bitvec_clusters_ref.py; only for inputs where every sum is sure"""
    acc, sure = fused_sums(q, X)
    assert sure.all(), "double rounding could blur this sum"
    return acc


def fuse_sensitive(seed, D=2):
    """(rows, queries, centres, clust_idx, raw queries): centres 0 and 1 lie at nearly the same distance from raw
    query 0, and their order under the reference's arithmetic (subtract, multiply, add, each rounded) differs from
    their order under a fused multiply-add (reversed, or equal under one and unequal under the other).  Seven other
    centres lie well apart behind them.  Each of the two clusters alone holds k rows, so query 0 visits one of them:
    the labels show which."""
    rs = np.random.RandomState(8000 + seed)
    far = (np.arange(7, dtype=np.float32)[:, None] + 5) * np.float32(3.0) * np.ones((1, D), np.float32)
    found = None
    for _ in range(400):
        q = rs.standard_normal(D).astype(np.float32)
        c0 = (q + rs.standard_normal(D)).astype(np.float32)
        # 2000 centres round the sphere about q through c0: rotations of c0 - q (in the first two coordinates)
        th = rs.uniform(0, 2 * np.pi, 2000)
        v = (c0 - q).astype(np.float64)
        c1 = np.repeat(c0[None, :], 2000, axis=0).astype(np.float64)
        c1[:, 0] = q[0] + np.cos(th) * v[0] - np.sin(th) * v[1]
        c1[:, 1] = q[1] + np.sin(th) * v[0] + np.cos(th) * v[1]
        c1 = c1.astype(np.float32)
        pf, sure = fused_sums(q, np.vstack([c0[None, :], c1]))
        pp = br.euclidean_no_sqrt(q, np.vstack([c0[None, :], c1]))
        plain = np.sign(pp[1:].astype(np.float64) - np.float64(pp[0]))
        fused = np.sign(pf[1:].astype(np.float64) - np.float64(pf[0]))
        hit = np.flatnonzero((plain != fused) & sure[1:] & sure[0])
        if len(hit):
            found = (q, c0, c1[hit[0]])
            break
    assert found is not None, "no pair found"
    q, c0, c1 = found
    for swap in (seed % 2, 1 - seed % 2):  # (a tie falls to the lower index: then one index order of the pair shows it)
        cen = np.vstack([c0[None, :], c1[None, :], far + q[None, :]]).astype(np.float32)
        if swap:
            cen[[0, 1]] = cen[[1, 0]]
        if cr.centre_order(cen, q)[0] != cr.centre_order(cen, q, euclidean_fused)[0]:
            break
    T = len(cen)
    nq = 3
    oq = rs.standard_normal((nq, D)).astype(np.float32)
    oq[0] = q
    rows, queries = crowd(rs, 200, 1, nq)
    sizes = [40, 40] + [17, 17, 17, 17, 17, 17, 18]
    idx = sizes_to_idx(rs, sizes)
    dp, df = br.euclidean_no_sqrt(q, cen), euclidean_fused(q, cen)
    assert max(dp[:2].max(), df[:2].max()) * 4 < min(dp[2:].min(), df[2:].min())  # the pair is nearest either way
    a = cr.query_clusters(rows, queries, cen, idx, oq, K_C, 1)
    b = cr.query_clusters(rows, queries, cen, idx, oq, K_C, 1, dist=euclidean_fused)
    assert not np.array_equal(a[0][0], b[0][0]), "a fused sum gives the same answer"
    assert cr.visited(cen, idx, q, K_C, 1)[0] != cr.visited(cen, idx, q, K_C, 1, dist=euclidean_fused)[0]
    return rows, queries, cen, idx, oq


NONFINITE = ("inf", "nan_query", "nan_centre", "nan_beside_tie", "nan_centre_small")


def nonfinite(kind):
    """(rows, queries, centres, clust_idx, raw queries, k, atleast) with centre distances that are +inf or NaN.
    inf: every third centre has one coordinate at +-3e19, so its squared distance is past FLT_MAX from finite inputs;
         the finite centres hold 16 rows in all, so k = 17 sends the walk in among the infinite ones, which tie.
    nan_query: raw query 0 has a NaN coordinate: all its distances are NaN.
    nan_centre: one centre has a NaN coordinate: one NaN among finite, distinct distances.
    nan_beside_tie: the same and two pairs of duplicated centres, one next to the NaN centre.
    nan_centre_small: T = 9, where std::sort is the insertion sort alone.
    T = 40 otherwise: past the introsort's threshold of 16, so the partition runs over the NaN."""
    rs = np.random.RandomState(9000 + NONFINITE.index(kind))
    T, D, nq, n = (9 if kind == "nan_centre_small" else 40), 4, 4, 900
    cen = rs.standard_normal((T, D)).astype(np.float32) * np.float32(37.5)
    oq = rs.standard_normal((nq, D)).astype(np.float32) * np.float32(37.5)
    rows, queries = bit_rows_c(rs, nq, n)
    k, atleast = K_C, 5
    idx = rs.randint(0, T, n).astype(np.int32)
    if kind == "inf":
        inf_c = np.arange(0, T, 3)
        for c in inf_c:
            cen[c, c % D] = np.float32(3e19) * (1 if c % 2 else -1)
        fin_c = np.setdiff1d(np.arange(T), inf_c)
        sizes = np.zeros(T, np.int64)
        sizes[fin_c[:16]] = 1
        sizes[inf_c] = (n - 16) // len(inf_c)
        sizes[inf_c[0]] += n - sizes.sum()
        idx = sizes_to_idx(rs, sizes)
        atleast = len(fin_c) + 4
    elif kind == "nan_query":
        oq[0, 2] = np.nan
    else:
        cen[T // 2, 1] = np.nan
        if kind == "nan_beside_tie":
            cen[T // 2 + 1] = cen[T // 2 - 1]
            cen[3] = cen[30]
    assert T > 16 or kind == "nan_centre_small"
    d = dists_of(cen, oq)
    if kind == "inf":
        assert np.isfinite(cen).all() and np.isfinite(oq).all() and not np.isnan(d).any()
        for q in range(nq):
            walk = cr.visited(cen, idx, oq[q], k, atleast)
            assert np.isinf(d[q][walk]).sum() >= 2 and np.isinf(d[q]).sum() == len(inf_c) > 2
    elif kind == "nan_query":
        assert np.isnan(d[0]).all() and np.isfinite(d[1:]).all()
    else:
        assert all(np.isnan(d[q]).sum() == 1 for q in range(nq))
        fin = [d[q][np.isfinite(d[q])] for q in range(nq)]
        assert all(len(np.unique(f)) == len(f) - (2 if kind == "nan_beside_tie" else 0) for f in fin)
    return rows, queries, cen, idx, oq, k, atleast


def sort_arrays():
    """the centre distances the plan's fallback sorts in the cases above, as (name, float32 array): the pair arrays
    tests/cpp/cluster_sort_test.cpp runs vaq::stdsort::sort_by<12, true> with ClusterLt on"""
    out = []
    for kind in NONFINITE:
        rows, queries, cen, idx, oq, k, atleast = nonfinite(kind)
        out += [("%s_q%d" % (kind, q), d) for q, d in enumerate(dists_of(cen, oq))]
    for T, D, nq in PLAN_TIE_SHAPES:
        rows, queries, cen, idx, oq, atleast = plan_shape(T, D, nq, True)
        out += [("ties_T%d_q%d" % (T, q), d) for q, d in enumerate(dists_of(cen, oq)[:2])]
    return out


# ---- D. seams -------------------------------------------------------------------------------------------------------

def small_chunks(n=100, W=3, nq=5, T=6, D=3):
    """(rows, queries, X uint8, XQ, centres, clust_idx) for the runs under a small dist_chunk_bytes: five queries whose
    cluster answers are pairwise different and whose first clusters differ"""
    rs = np.random.RandomState(34)
    rows = near(rs, words(rs, 1, W)[0], n, 12)
    queries = near(rs, rows[0], nq, 8)
    X = rs.randint(0, 4, (n, D)).astype(np.uint8)
    cen = rs.permutation(np.array([[a, b, c] for a in (0, 3) for b in (0, 3) for c in (0, 3)], np.float32))[:T]
    XQ = (cen[:nq] + rs.randint(0, 2, (nq, D)) * (np.where(cen[:nq] > 0, -1, 1))).astype(np.float32)
    idx = rs.randint(0, T, n).astype(np.int32)
    first = [int(cr.centre_order(cen, XQ[q])[0]) for q in range(nq)]
    assert len(set(first)) == nq, "two queries share their first cluster"
    assert distinct_answers(*cr.query_clusters(rows, queries, cen, idx, XQ, 17, 2))
    assert distinct_answers(*cr.query_rerank_clusters(rows, queries, cen, idx, X, XQ, 5, 3, 2))
    # the second chunk (queries 3, 4) answered from the raw queries of the first (0, 1) is another answer
    a = cr.query_clusters(rows, queries[3:], cen, idx, XQ[3:], 17, 2)
    b = cr.query_clusters(rows, queries[3:], cen, idx, XQ[:2], 17, 2)
    assert all(not np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    a = cr.query_rerank_clusters(rows, queries[3:], cen, idx, X, XQ[3:], 5, 3, 2)
    b = cr.query_rerank_clusters(rows, queries[3:], cen, idx, X, XQ[:2], 5, 3, 2)
    assert all(not np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    return rows, queries, X, XQ, cen, idx


def seam(n=64, T=4, D=4, k=3, k_rr=2, factor=2):
    """(rows, base bit queries, X uint8, base raw queries, centres, clust_idx, want of query_clusters, want of
    query_rerank_clusters): W = 1; the bit queries and the raw queries repeat together with period 7.  Bit queries, raw
    queries and answers are each pairwise different over the seven residues, and every answer changes when the raw
    queries are rolled by one against the bit queries -- so a wrong d_oq offset shows apart from a wrong d_bq one."""
    for seed in range(200):
        rs = np.random.RandomState(3500 + seed)
        rows = words(rs, n, 1)
        base = near(rs, rows[9], PERIOD, 9)
        X = rs.randint(0, 256, (n, D)).astype(np.uint8)
        XQ = rs.randint(0, 256, (PERIOD, D)).astype(np.float32)
        cen = rs.randint(0, 256, (T, D)).astype(np.float32)
        idx = sizes_to_idx(rs, [n // T] * T)
        want = cr.query_clusters(rows, base, cen, idx, XQ, k, 1)
        want_rr = cr.query_rerank_clusters(rows, base, cen, idx, X, XQ, k_rr, factor, 1)
        rolled = np.roll(XQ, 1, axis=0)
        other = cr.query_clusters(rows, base, cen, idx, rolled, k, 1)
        other_rr = cr.query_rerank_clusters(rows, base, cen, idx, X, rolled, k_rr, factor, 1)
        swapped = cr.query_clusters(rows, np.roll(base, 1, axis=0), cen, idx, XQ, k, 1)
        # a chunk that reads the raw queries (or the bit queries) from the start of the array: the queries behind the
        # seam, residues QUERY_CHUNK % 7 onwards, meet those of residues 0 onwards
        behind = (QUERY_CHUNK + np.arange(5)) % PERIOD
        no_oq = cr.query_clusters(rows, base[behind], cen, idx, XQ[:5], k, 1)
        no_oq_rr = cr.query_rerank_clusters(rows, base[behind], cen, idx, X, XQ[:5], k_rr, factor, 1)
        no_bq = cr.query_clusters(rows, base[:5], cen, idx, XQ[behind], k, 1)
        if (distinct_answers(*want) and distinct_answers(*want_rr)
                and all(not np.array_equal(a, b) for a, b in zip(want[0], other[0]))
                and all(not np.array_equal(a, b) for a, b in zip(want_rr[0], other_rr[0]))
                and all(not np.array_equal(a, b) for a, b in zip(want[0], swapped[0]))
                and all(not np.array_equal(a, b) for a, b in zip(want[0][behind], no_oq[0]))
                and all(not np.array_equal(a, b) for a, b in zip(want_rr[0][behind], no_oq_rr[0]))
                and all(not np.array_equal(a, b) for a, b in zip(want[0][behind], no_bq[0]))):
            break
    else:
        raise AssertionError("no seed gives seven answers that differ and follow both kinds of query")
    assert len({tuple(b) for b in base.tolist()}) == PERIOD and len({tuple(x) for x in XQ.tolist()}) == PERIOD
    assert QUERY_CHUNK % PERIOD and (want[0] >= 0).all() and (want_rr[0] >= 0).all()
    return rows, base, X, XQ, cen, idx, want, want_rr


# ---- E. state -------------------------------------------------------------------------------------------------------

def state_steps():
    """[(rows or None, centres, clust_idx)]: what one handle is given in turn -- T = 300, 3, 300 again, another D, then
    fewer rows with other cluster sizes (rows None: the rows stay).  Plus the queries and, per D, the raw queries."""
    rs = np.random.RandomState(77)
    rows, queries = crowd(rs, 900, 2, 6)
    fewer = np.ascontiguousarray(rows[rs.choice(900, 333, replace=False)])
    oq = {D: rs.standard_normal((6, D)).astype(np.float32) for D in (4, 9)}
    steps, held = [], None
    for T, D, r in ((300, 4, rows), (3, 4, None), (300, 4, None), (40, 9, None), (7, 9, fewer), (300, 4, None)):
        held = held if r is None else r
        cen = rs.standard_normal((T, D)).astype(np.float32)
        steps.append((r, cen, rs.randint(0, T, len(held)).astype(np.int32)))
    assert [len(s[1]) for s in steps] == [300, 3, 300, 40, 7, 300] and [len(s[2]) for s in steps] == [900] * 4 + [333] * 2
    return steps, queries, oq
