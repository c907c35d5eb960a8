"""Case builders and CPU models for tests/test_ti_shapes_cpu.py and tests/test_ti_shapes_gpu.py: the
index-side regroup (ti_assign_kernel .. ti_bounds_kernel) and the per-query plan (ti_plan_kernel) of
vaq_amd/csrc/vaq_ti.hip at the summation orders and launch tiers the scan tests do not bring with them.

1. Twin-centre cases.  fvec_L2sqr_ny (utils/Math.hpp:38-171) sums d in {1, 2, 4, 8, 12} in its SSE orders
   and everything else sequentially.  A twin case makes that order decide the answer:
     * codebook and query values are multiples of 2^-4 in [-4, 4];
     * an anchor x is the decoded first `seg` codes of some rows (many rows share it) or the first d dims
       of a query; anchors are kept more than 2 * sqrt(d) * 2^-3 + 2^-4 apart;
     * its twin centres are c = x - delta and c' = x - perm(delta), delta_j a multiple of 2^-20 with
       |delta_j| < 2^-3: c, c', x - c and x - c' are exact in fp32, the squares are the same multiset, the
       true squared distances are equal, and the fp32 sums differ only through the order of addition.
       The strict `<` on the square roots then sends the anchor's rows -- and a query sitting on it -- to
       one twin or the other;
     * every centre is a twin, so the nearest two centres of an anchor are always its own pair
       (check_twins_nearest).
   d = 1 and d = 2 cannot disagree (one term; one addition): they are branch coverage only.
2. Tier cases: one per edge of ti_assign_lds, which is restated here (assign_tier).
3. Plan cases: T in {1, 2, 3, 511, 512, 513, 2000, 4096} over 8 byte codes.
"""
from __future__ import annotations

import numpy as np

from oracle import pyoracle as po
from test_ti import ti_case, visited_dists

F32 = np.float32


# ------------------------------------------------------------------ summation orders --
def _terms(x, Y):
    """ElementOpL2::op per dimension: (x_j - y_j)^2 in fp32, one column per dimension."""
    t = np.asarray(x, F32)[None, :] - np.asarray(Y, F32)
    return t * t


def l2_sequential(x, Y):
    """fvec_L2sqr_ref: res = 0; res += t_j, j ascending."""
    t = _terms(x, Y)
    acc = np.zeros(t.shape[0], F32)
    for j in range(t.shape[1]):
        acc = acc + t[:, j]
    return acc


def l2_lanes(x, Y):
    """Four lanes, lane l sums the terms j = l, l + 4, ... in turn, then (a0 + a1) + (a2 + a3): the SSE
    kernels of d = 4, 8, 12 -- and what a kernel would compute that took that shape for every d % 4 == 0."""
    t = _terms(x, Y)
    d = t.shape[1]
    assert d % 4 == 0
    a = [t[:, l] for l in range(4)]
    for j in range(4, d):
        a[j % 4] = a[j % 4] + t[:, j]
    return (a[0] + a[1]) + (a[2] + a[3])


def l2_tree3(x, Y):
    """d = 3 only: t0 + (t1 + t2).  (Four lanes with an empty fourth, (t0 + t1) + (t2 + 0), ARE the sequential
    sum at d = 3, so the pairwise model that can be told apart there is the other tree.)"""
    t = _terms(x, Y)
    assert t.shape[1] == 3
    return t[:, 0] + (t[:, 1] + t[:, 2])


def l2_ref_order(x, Y):
    """fvec_L2sqr_ny as the reference computes it: the third statement of it next to oracle/vaq_oracle.c
    and vaq_ti.hip's l2sqr_ref_order, checked against both the oracle and (where built) the compiled
    reference in test_ti_shapes_cpu.py."""
    d = np.asarray(Y).shape[1]
    if d == 2:
        t = _terms(x, Y)
        return t[:, 0] + t[:, 1]
    if d in (4, 8, 12):
        return l2_lanes(x, Y)
    return l2_sequential(x, Y)


def wrong_order(d):
    """The summation order a kernel would use that had the branch of this d wrong (None: no other order)."""
    if d in (4, 8, 12):
        return l2_sequential
    if d == 3:
        return l2_tree3
    if d == 16:
        return l2_lanes
    return None


# ------------------------------------------------------------------ twin cases --
# d -> (seg, L, bits, seed).  [8] * 8 is the byte-code layout, [8] * 4 bit-packed (one dword per row).
# Seeds are chosen in test_ti_shapes_cpu.py's terms: see test_twin_cases_have_teeth.
TWIN_CASES = {
    1: (1, 1, [8] * 8, 11),
    2: (1, 2, [8] * 4, 12),
    3: (3, 1, [8] * 4, 78),
    4: (2, 2, [8] * 8, 17),
    8: (2, 4, [8] * 4, 14),
    12: (3, 4, [8] * 8, 20),
    16: (4, 4, [8] * 8, 12),
}
TWIN_N = 4001
TWIN_NQ = 32
TWIN_ROW_ANCHORS = 24    # anchors that many rows share; a query sits on each
TWIN_QUERY_ANCHORS = 8   # anchors of a query alone (rows come to their twins by chance)
TWIN_T = 2 * (TWIN_ROW_ANCHORS + TWIN_QUERY_ANCHORS)


def _grid(rng, shape):
    return (rng.integers(-64, 65, size=shape) / 16.0).astype(F32)


def _spread(rng, cand, n, sep):
    """n rows of cand, pairwise more than sep apart (greedy over a random order)."""
    out = []
    for i in rng.permutation(len(cand)):
        if all(np.sqrt(((cand[i].astype(np.float64) - cand[j]) ** 2).sum()) > sep for j in out):
            out.append(int(i))
            if len(out) == n:
                return out
    raise AssertionError(f"only {len(out)} of {n} anchors more than {sep} apart")


def twin_case(d, seed=None):
    seg, L, bits, default_seed = TWIN_CASES[d]
    seed = default_seed if seed is None else seed
    assert seg * L == d
    rng = np.random.default_rng(7000 + seed)
    M, N, nq = len(bits), TWIN_N, TWIN_NQ
    D = M * L
    cents = [_grid(rng, (1 << b, L)) for b in bits]
    codes = np.stack([rng.integers(0, 1 << b, size=N) for b in bits], 1).astype(np.uint16)
    X = _grid(rng, (nq, D))
    # anchors: decoded code prefixes, far enough apart that another pair is never nearer than one's own
    n_anchor = TWIN_ROW_ANCHORS + TWIN_QUERY_ANCHORS
    dmax = 2.0 ** -3 if d > 1 else 2.0 ** -6  # (d = 1: [-4, 4] has no room for 32 anchors 5/16 apart)
    sep = 2 * np.sqrt(d) * dmax + 2.0 ** -4
    prefixes = np.stack([rng.integers(0, 1 << bits[s], size=4096) for s in range(seg)], 1)
    decoded = np.concatenate([cents[s][prefixes[:, s]] for s in range(seg)], axis=1)
    keep = _spread(rng, decoded, n_anchor, sep)
    anchors = decoded[keep]
    # rows: 16..47 per row anchor carry its prefix, at scattered places; the other rows stay random
    perm_rows = rng.permutation(N)
    at = 0
    anchor_rows = []
    for a in range(TWIN_ROW_ANCHORS):
        n_a = int(rng.integers(16, 48))
        rows = np.sort(perm_rows[at:at + n_a])
        at += n_a
        codes[rows, :seg] = prefixes[keep[a]]
        anchor_rows.append(rows)
    # queries: query a sits on anchor a (the last 8 on anchors of their own)
    assert nq == n_anchor
    X[:, :d] = anchors
    # twin centres, the pairs in shuffled places so that the lower index is not always c
    lim = int(dmax * 2 ** 20)
    clusters = np.empty((TWIN_T, d), F32)
    slots = rng.permutation(TWIN_T)
    twins = np.empty((n_anchor, 2), np.int64)
    for a in range(n_anchor):
        delta = (rng.integers(-lim + 1, lim, size=d) / 2.0 ** 20)
        t1, t2 = sorted(slots[2 * a:2 * a + 2])
        clusters[t1] = (anchors[a].astype(np.float64) - delta).astype(F32)
        clusters[t2] = (anchors[a].astype(np.float64) - delta[rng.permutation(d)]).astype(F32)
        twins[a] = (t1, t2)
        for t in (t1, t2):  # exact: x - c gives delta back
            back = anchors[a].astype(np.float64) - clusters[t].astype(np.float64)
            assert np.array_equal((anchors[a] - clusters[t]).astype(np.float64), back)
            assert np.array_equal(np.sort(back), np.sort(delta))
    return dict(D=D, M=M, L=L, bits=list(bits), cents=cents, X=X, codes=codes, eig=None, clusters=clusters, seg=seg,
                T=TWIN_T, d=d, anchors=anchors, anchor_rows=anchor_rows, twins=twins)


def check_twins_nearest(c):
    """Every anchor's two nearest centres are its own pair, by a margin far above rounding."""
    for a in range(len(c["anchors"])):
        dist = np.sqrt(((c["anchors"][a].astype(np.float64) - c["clusters"].astype(np.float64)) ** 2).sum(1))
        own = dist[c["twins"][a]]
        rest = np.delete(dist, c["twins"][a])
        assert own[0] == own[1] and (c["d"] == 1 or own[0] > 0)
        assert rest.min() > own[0] + 2.0 ** -5, (a, own, rest.min())


def decode_rows(c):
    seg = c["seg"]
    return np.concatenate([c["cents"][s][c["codes"][:, s].astype(np.int64)] for s in range(seg)], axis=1)


def model_grouping(c, l2):
    """VAQ::clusterTI's grouping (VAQ.cpp:926-996) with l2 in place of fvec_L2sqr_ny: the nearest centre by
    sqrt, first minimum; members farthest first, equal distances by ascending row.
    -> (assign[N], member[N], start[T + 1], xcc[N])"""
    Xr = decode_rows(c)
    T = c["clusters"].shape[0]
    uniq, inv = np.unique(Xr, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    dist = np.sqrt(np.stack([l2(u, c["clusters"]) for u in uniq]))  # [unique rows][T]
    assign_u = np.argmin(dist, axis=1)
    assign = assign_u[inv]
    xcc = dist[np.arange(len(uniq)), assign_u][inv].astype(F32)
    member = np.lexsort((np.arange(len(assign)), -xcc.astype(np.float64), assign)).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=T))]).astype(np.int32)
    return assign, member, start, xcc


def model_query_order(c, l2):
    """VAQ::search's TI branch (VAQ.cpp:799-826) with l2: -> (qcc[nq][T], order[nq][T]), equal distances by
    ascending cluster."""
    d, T = c["d"] if "d" in c else c["seg"] * c["L"], c["clusters"].shape[0]
    qcc = np.sqrt(np.stack([l2(x[:d], c["clusters"]) for x in c["X"]])).astype(F32)
    order = np.stack([np.lexsort((np.arange(T), qcc[q])) for q in range(len(qcc))]).astype(np.int32)
    return qcc, order


def visiting_rows(member, start, order_q, k=None):
    """Original rows in the order searchTriangleInequality meets them for one query (the first k)."""
    rows = np.concatenate([member[start[t]:start[t + 1]] for t in order_q] + [np.empty(0, np.int32)])
    return rows if k is None else rows[:k]


def model_first_k(c, l2, k):
    """The label sets NNMethod.TI without EA returns under l2: the first k rows of each visiting order."""
    _, member, start, _ = model_grouping(c, l2)
    _, order = model_query_order(c, l2)
    return [set(visiting_rows(member, start, order[q], k).tolist()) for q in range(len(order))]


def oracle_grouping(c, nthreads=1):
    return po.cluster_ti(c["codes"], c["cents"], c["clusters"], c["seg"], nthreads=nthreads)


def oracle_assign(ti):
    """cluster of every original row, from the oracle's member / start."""
    out = np.empty(len(ti["member"]), np.int64)
    out[ti["member"]] = np.repeat(np.arange(len(ti["start"]) - 1), np.diff(ti["start"]))
    return out


def oracle_orders(c):
    d = c["seg"] * c["L"]
    both = [po.ti_query_order(x[:d], c["clusters"]) for x in c["X"]]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def twin_ks(c, ti, order):
    """k = 1 and, for the first two queries, the size of the cluster each visits first -1, +0, +1."""
    ks = {1}
    for q in (0, 1):
        first = next(t for t in order[q] if ti["start"][t + 1] > ti["start"][t])
        size = int(ti["start"][first + 1] - ti["start"][first])
        ks |= {size - 1, size, size + 1}
    return sorted(k for k in ks if k >= 1)


def check_cut_points(ti, qcc, order, ks):
    """The first k rows of a visiting order are one well-defined set under the two documented tie rules --
    equal qToCCDist by ascending cluster, equal mCodeToCCDist by ascending row -- which both the oracle and
    the kernels (the plan's (distance, cluster) key; the stable radix sort) follow: wherever a cut falls
    inside a run of equal keys, that run is in ascending order."""
    member, start, xcc = ti["member"], ti["start"], ti["code2cc"]
    for q in range(len(order)):
        o = order[q]
        same = qcc[q][o][:-1] == qcc[q][o][1:]
        assert np.all(o[:-1][same] < o[1:][same]), q
        rows = visiting_rows(member, start, o)
        cl = np.repeat(o, np.diff(start)[o])
        for k in ks:
            if 0 < k < len(rows) and cl[k - 1] == cl[k] and xcc[rows[k - 1]] == xcc[rows[k]]:
                lo = k - 1
                while lo > 0 and cl[lo - 1] == cl[k] and xcc[rows[lo - 1]] == xcc[rows[k]]:
                    lo -= 1
                hi = k
                while hi + 1 < len(rows) and cl[hi + 1] == cl[k] and xcc[rows[hi + 1]] == xcc[rows[k]]:
                    hi += 1
                assert np.all(np.diff(rows[lo:hi + 1]) > 0), (q, k)


def twin_teeth(c):
    """How many anchors / queries / answers the wrong summation order would change (conditions on the
    inputs): -> (anchors assigned to the other twin, queries ranking their twins the other way, queries
    whose non-EA answer differs at some k of twin_ks)."""
    wrong = wrong_order(c["d"])
    ti = oracle_grouping(c)
    o_assign = oracle_assign(ti)
    qcc, order = oracle_orders(c)
    w_assign, w_member, w_start, _ = model_grouping(c, wrong)
    _, w_order = model_query_order(c, wrong)
    anchors = 0
    for a, rows in enumerate(c["anchor_rows"]):
        assert len(set(o_assign[rows].tolist())) == 1 and o_assign[rows[0]] in c["twins"][a]
        assert w_assign[rows[0]] in c["twins"][a]
        anchors += int(o_assign[rows[0]] != w_assign[rows[0]])
    queries = 0
    for q in range(len(order)):
        assert set(order[q][:2].tolist()) == set(c["twins"][q].tolist()) == set(w_order[q][:2].tolist())
        queries += int(order[q][0] != w_order[q][0])
    answers = set()
    for k in twin_ks(c, ti, order):
        for q in range(len(order)):
            if set(visiting_rows(ti["member"], ti["start"], order[q], k).tolist()) != \
                    set(visiting_rows(w_member, w_start, w_order[q], k).tolist()):
                answers.add(q)
    return anchors, queries, len(answers)


# ------------------------------------------------------------------ assign tiers --
ASSIGN_LDS_SOFT = 48 * 1024    # ti_assign_lds halves the rows per workgroup (256 -> 64) to stay within this
ASSIGN_LDS_MAX = 128 * 1024    # ... and above this the decoded rows go to a global scratch tile
ASSIGN_SCRATCH_GRID = 2048     # workgroups of the scratch tier; more rows are served by its grid-stride loop
MAX_TI_DIMS = 1024             # check_ti_shape (vaqhip_codes.cpp)


def assign_tier(d):
    """ti_assign_lds (vaq_ti.hip) restated: -> (rows per workgroup, LDS bytes; 0 = global scratch)."""
    R = 256
    while R > 64 and R * d * 4 > ASSIGN_LDS_SOFT:
        R >>= 1
    b = R * d * 4
    return R, (b if b <= ASSIGN_LDS_MAX else 0)


# name: (d, seg, L, N, T, what the case is meant to hit: rows per workgroup, LDS bytes, trips of the loop)
# All over bits = [8] * 4 (bit-packed rows of one dword, D = 4 * L).
TIER_CASES = {
    "d48_r256": (48, 4, 12, 257, 5, (256, 48 * 1024, 1)),       # exactly 48 KB; a second workgroup of one row
    "d49_r128": (49, 1, 49, 129, 6, (128, 128 * 49 * 4, 1)),
    "d49_one_row": (49, 1, 49, 1, 4, (128, 128 * 49 * 4, 1)),   # N smaller than one workgroup's rows, and than k
    "d96_r128": (96, 2, 48, 200, 7, (128, 48 * 1024, 1)),
    "d97_r64": (97, 1, 97, 200, 8, (64, 64 * 97 * 4, 1)),
    "d192_r64": (192, 4, 48, 65, 4, (64, 48 * 1024, 1)),
    "d193_above48k": (193, 1, 193, 65, 5, (64, 64 * 193 * 4, 1)),
    "d512_lds_max": (512, 4, 128, 300, 6, (64, 128 * 1024, 1)),
    "d513_scratch": (513, 3, 171, 300, 7, (64, 0, 1)),
    "d1024_scratch": (1024, 4, 256, 130, 8, (64, 0, 1)),
    # 2049 + 1 workgroups' worth of rows over a grid of 2048: the second trip of the grid-stride loop, its
    # last workgroup one row short of two.  2048 * 64 * 520 * 4 B = 273 MB of scratch on the device.
    "d520_second_trip": (520, 4, 130, 2048 * 64 + 65, 4, (64, 0, 2)),
}
TIER_REFUSED = ("d1025", 1025, 1, 1025)  # d, seg, L: one dimension more than check_ti_shape allows
TIER_BITS = [8] * 4


def tier_trips(d, N):
    R, lds = assign_tier(d)
    wgs = -(-N // R)
    return -(-wgs // ASSIGN_SCRATCH_GRID) if lds == 0 else 1


def tier_case(name):
    d, seg, L, N, T, _ = TIER_CASES[name]
    return ti_case(4100 + d + N % 97, 4 * L, TIER_BITS, N, 4, T, seg)


def tier_ks(N):
    return sorted({1, 5, min(N, 64) - 1 if N > 2 else 1, 37})


# ------------------------------------------------------------------ plan cases --
PLAN_T = (1, 2, 3, 511, 512, 513, 2000, 4096)
PLAN_BITS = [8] * 8
PLAN_NQ = 9
PLAN_THREADS = 256  # TI_PLAN_THREADS: one pass of the bitonic network covers Tp / 2 <= 256 pairs
MAX_TI_CLUSTERS = 4096


def plan_rows(T):
    return min(3 * T + 61, 12000)


def plan_case(T, seed=0):
    """Continuous data over 8 byte codes, D = 32, seg = 4 (d = 16: the sequential branch), about three rows
    per cluster.  From T = 511 on the centres are T distinct rows (ti_case draws with replacement: at
    T = 4096 of 12 000 rows some 700 centres would be copies of another, their clusters empty)."""
    N = plan_rows(T)
    c = ti_case(5200 + T + 7919 * seed, 32, PLAN_BITS, N, PLAN_NQ, T, 4)
    if T >= 511:
        pick = np.random.default_rng(5300 + T + seed).permutation(N)[:T]
        c["clusters"] = np.ascontiguousarray(
            np.concatenate([c["cents"][s][c["codes"][pick, s].astype(np.int64)] for s in range(4)], axis=1), F32)
    return c


def plan_visits(T):
    """1.0, 0.3, and the smallest that still visits one cluster: int(float(T) * visit) == 1 (VAQ.cpp:1548)."""
    least = min(1.0, 1.5 / T)
    assert least >= 1.0 or int(F32(T) * F32(least)) == 1
    return [1.0, 0.3] + ([least] if least < 1.0 else [])


def plan_tp(T):
    Tp = 2
    while Tp < T:
        Tp <<= 1
    return Tp


EXACT_T = (600, 4096)


def exact_case(T):
    """plan_case with queries none of which has two clusters at one qToCCDist.  (At T = 4096 the 8.4 M pairs
    of a query's distances, all within a few binades of fp32, collide about once per query: the queries are
    the first PLAN_NQ of 64 drawn for which the oracle finds no such pair.)"""
    c = plan_case(T, seed=1)
    rng = np.random.default_rng(5400 + T)
    cand = (rng.normal(size=(64, c["D"])) * 30.0).astype(F32)
    keep = [x for x in cand if len(np.unique(po.ti_query_order(x[:16], c["clusters"])[0])) == T][:PLAN_NQ]
    assert len(keep) == PLAN_NQ, len(keep)
    c["X"] = np.ascontiguousarray(np.stack(keep))
    return c


def check_no_ties(c, ti, combos):
    """What lets option "exact_ties" and the default answer be compared label for label: per query no two
    clusters at one qToCCDist, inside a cluster no two members at one mCodeToCCDist, and for every
    (k, visit, ea) of combos the oracle's k + 1 smallest distances differ and are the k-min of the rows
    it may visit (the reference's fp32 pruning lost none)."""
    qcc, order = oracle_orders(c)
    for q in range(len(qcc)):
        assert len(np.unique(qcc[q])) == len(qcc[q]), q
    xcc, member, start = ti["code2cc"], ti["member"], ti["start"]
    for t in range(len(start) - 1):
        x = xcc[member[start[t]:start[t + 1]]]
        assert len(np.unique(x)) == len(x), t
    for k, visit, ea in combos:
        if ea:
            alld = np.sort(visited_dists(c, ti, visit, k), axis=1)[:, :k + 1]
            assert np.all(alld[:, :-1] < alld[:, 1:]) and np.all(np.isfinite(alld)), (k, visit)
            _, od, _ = po.search_ti(c["X"], c["cents"], ti, k, visit=visit, projected=True)
            assert np.array_equal(od.view(np.uint32), alld[:, :k].view(np.uint32)), (k, visit)
        else:
            lut = [po.create_lut(x, c["cents"], 8) for x in c["X"]]
            for q in range(len(order)):
                rows = visiting_rows(member, start, order[q], k)
                dd = po.all_dists(lut[q], c["codes"][rows])
                assert len(rows) == k and len(np.unique(np.sqrt(dd))) == k, (q, k)
