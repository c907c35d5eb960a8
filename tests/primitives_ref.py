"""Plain numpy references for the first-round primitives of vaq_front.hip, vaq_codes.hip and vaq_merge.hip
(projection, encoder, the old refine, the k-min merge) and the input generators the edge tests share.

Every operation has two references:

  * an EXACT one -- float32 arithmetic in the order include/vaqhip.h documents, vectorised over rows
    with the inner index sequential, so numpy rounds each operation exactly as the kernel does;
  * a FLOAT64 one, as a second, independent guard.

The float64 bound (derived, not tuned).  A distance is  sum_j fl(fl(x_j - y_j)^2)  added one by one in
float32.  With u = 2**-24: the subtraction, the square and each of the n - 1 additions contribute a
factor (1 + d), |d| <= u, and every term is non-negative, so to first order

    |d32 - d64| <= (n + 2) * u * d64        [+ n * 2**-149 for squares that underflow]

where d64 is the same sum in float64 (whose own error, ~n * 2**-53, is far below u).  The projection
has signed terms, so no such relative bound exists; there the project's stated bar is used:
|got - ref64| <= 1e-4 * max|ref64|  (tests/test_parity_gpu.py::test_projection_tolerance).

For the encoder float64 may legitimately pick another centroid at a near tie, so the guard is on the
distance, not the code: with g the code under test and m64 the float64 minimum over the codebook,
d32(g) <= d32(argmin64) <= m64 (1 + (L + 2) u)  and  d32(g) >= d64(g) (1 - (L + 2) u) >= m64 (1 - (L + 2) u).
"""
from __future__ import annotations

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
U32 = 2.0 ** -24


def sum_bound(n: int, d64):
    """|sequential float32 sum of n squared differences - the float64 one| is at most this."""
    return (n + 2) * U32 * np.asarray(d64, np.float64) + n * 2.0 ** -149


def sort_tie_runs(labels, dists):
    """labels with every run of bit-equal distances sorted by label (the oracle's heap leaves ties in
    heap order; the GPU's contract is (distance, label))."""
    out = np.array(labels, copy=True)
    d = np.ascontiguousarray(dists, np.float32).view(np.uint32)
    for q in range(out.shape[0]):
        cuts = np.r_[0, np.nonzero(d[q, 1:] != d[q, :-1])[0] + 1, d.shape[1]]
        for a, b in zip(cuts[:-1], cuts[1:]):
            out[q, a:b] = np.sort(out[q, a:b])
    return out


def same_bits(a, b) -> bool:
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def same_bits_or_nan(a, b) -> bool:
    """Bit equality, except that two NaNs are equal whatever their sign and payload: the NaN an
    operation GENERATES (inf - inf) is 0xffc00000 on x86 and 0x7fc00000 on the GPU."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ------------------------------------------------------------------------------------------ projection
def _fma32(x, y, acc):
    """fl32(x * y + acc) with ONE rounding, for float32 arrays.  The product of two float32 is exact in
    float64; the float64 sum is made exact-or-odd (TwoSum gives its error; an inexact sum whose last bit
    is even moves to its odd neighbour on the error's side), and rounding an odd-rounded float64 to
    float32 equals rounding the exact value (29 spare bits)."""
    p = x.astype(np.float64) * y.astype(np.float64)
    a = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + a
        bb = s - p
        err = (p - (s - bb)) + (a - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def project32(X, E):
    """VAQ::ProjectOnEigenVectors as the kernels and the oracle spell it: out[r, c] is one fma chain
    acc = fma(X[r, j], E[j, c], acc) over j ascending from acc = 0."""
    X = np.ascontiguousarray(X, np.float32)
    E = np.ascontiguousarray(E, np.float32)
    acc = np.zeros((X.shape[0], E.shape[1]), np.float32)
    for j in range(X.shape[1]):
        acc = _fma32(X[:, j:j + 1], E[j:j + 1, :], acc)
    return acc


def project64(X, E):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(X, np.float64) @ np.asarray(E, np.float64)


# --------------------------------------------------------------------------------------------- encoder
def sqdist32(Xs, C):
    """[n, K] float32: dist = 0; dist += t * t for j ascending, t = x_j - c_j; multiply and add unfused."""
    Xs = np.ascontiguousarray(Xs, np.float32)
    C = np.ascontiguousarray(C, np.float32)
    d = np.zeros((Xs.shape[0], C.shape[0]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(Xs.shape[1]):
            t = Xs[:, j:j + 1] - C[None, :, j]
            d = d + t * t
    return d


def sqdist64(Xs, C):
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(Xs, np.float64)[:, None, :] - np.asarray(C, np.float64)[None, :, :]
        return (t * t).sum(-1)


def argmin_strict(d):
    """best = 0, bsf = FLT_MAX; for c ascending: if d[c] < bsf: take it.  The first minimum wins; a row
    whose distances are all NaN, infinite or FLT_MAX keeps code 0."""
    ok = d < FLT_MAX  # False for NaN
    return np.argmin(np.where(ok, d, np.float32(np.inf)), axis=1).astype(np.uint16)


def encode32(Xp, cents, chunk=1 << 16):
    """VAQ::encodeImpl as the oracle restates it (oracle/vaq_oracle.c, vo_encode)."""
    Xp = np.ascontiguousarray(Xp, np.float32)
    n = Xp.shape[0]
    codes = np.empty((n, len(cents)), np.uint16)
    off = 0
    for s, C in enumerate(cents):
        L = C.shape[1]
        step = max(1, min(n, (chunk * 256) // max(C.shape[0], 1)))
        for r in range(0, n, step):
            codes[r:r + step, s] = argmin_strict(sqdist32(Xp[r:r + step, off:off + L], C))
        off += L
    return codes


def encode64(Xp, cents):
    """(codes, minima): float64 argmin per subspace and the float64 minimum itself, [n, M] each."""
    Xp = np.asarray(Xp, np.float32)
    n = Xp.shape[0]
    codes = np.empty((n, len(cents)), np.int64)
    mins = np.empty((n, len(cents)), np.float64)
    off = 0
    for s, C in enumerate(cents):
        L = C.shape[1]
        d = sqdist64(Xp[:, off:off + L], C)
        codes[:, s] = np.argmin(d, axis=1)
        mins[:, s] = d.min(axis=1)
        off += L
    return codes, mins


def code_dist32(Xp, cents, codes):
    """float32 sequential distance of each row to the centroid its code names, [n, M]."""
    Xp = np.ascontiguousarray(Xp, np.float32)
    out = np.empty(codes.shape, np.float32)
    off = 0
    for s, C in enumerate(cents):
        L = C.shape[1]
        y = np.asarray(C, np.float32)[np.asarray(codes)[:, s].astype(np.int64)]
        d = np.zeros(Xp.shape[0], np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(L):
                t = Xp[:, off + j] - y[:, j]
                d = d + t * t
        out[:, s] = d
        off += L
    return out


# ------------------------------------------------------------------------------------------ old refine
def _topk_pairs(d, lab, k):
    """k smallest (distance bits, label) pairs; unfilled slots -1 / FLT_MAX.  Distances are >= 0, so
    the order of their bit patterns is the order of their values."""
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | lab.astype(np.int64).astype(np.uint64)
    o = np.argsort(key, kind="stable")[:k]
    out_l = np.full(k, -1, np.int32)
    out_d = np.full(k, FLT_MAX, np.float32)
    out_l[:o.size] = lab[o]
    out_d[:o.size] = d[o]
    return out_l, out_d


def refine32(Xq, Xt, cand, k):
    """VAQ::refine (vaqhip_refine*): sequential float32 sum per candidate; a candidate is admitted when
    dist < FLT_MAX (so NaN and overflow never are); negative labels are skipped; duplicates are kept;
    the result is the k smallest by (distance bits, label)."""
    Xq = np.ascontiguousarray(Xq, np.float32)
    Xt = np.ascontiguousarray(Xt, np.float32)
    cand = np.asarray(cand, np.int32)
    nq, R = cand.shape
    labels = np.empty((nq, k), np.int32)
    dists = np.empty((nq, k), np.float32)
    for q in range(nq):
        lab = cand[q][cand[q] >= 0]
        y = Xt[lab]
        d = np.zeros(lab.size, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(Xq.shape[1]):
                t = Xq[q, j] - y[:, j]
                d = d + t * t
        ok = d < FLT_MAX
        labels[q], dists[q] = _topk_pairs(d[ok], lab[ok], k)
    return labels, dists


def refine64_dists(Xq, Xt, labels):
    """float64 squared distance of every returned label (NaN where the label is -1), [nq, k]."""
    Xq = np.asarray(Xq, np.float64)
    Xt = np.asarray(Xt, np.float64)
    labels = np.asarray(labels)
    out = np.full(labels.shape, np.nan)
    for q in range(labels.shape[0]):
        ok = labels[q] >= 0
        t = Xq[q][None, :] - Xt[labels[q][ok]]
        out[q, ok] = (t * t).sum(-1)
    return out


# ----------------------------------------------------------------------------------------------- merge
def merge_ref(dist_lists, label_lists, k):
    """[n_lists, nq, k'] lists -> per query the k smallest by (distance bits, label) over the entries
    with label >= 0; unfilled slots -1 / FLT_MAX."""
    d = np.asarray(dist_lists, np.float32)
    l = np.asarray(label_lists, np.int32)
    nq = d.shape[1]
    labels = np.empty((nq, k), np.int32)
    dists = np.empty((nq, k), np.float32)
    for q in range(nq):
        dq = np.ascontiguousarray(d[:, q].reshape(-1))
        lq = l[:, q].reshape(-1)
        ok = lq >= 0
        labels[q], dists[q] = _topk_pairs(np.ascontiguousarray(dq[ok]), lq[ok], k)
    return labels, dists


# ------------------------------------------------------------------------------------ input generators
MERGE_TIE_QUERY = 5    # k-th and (k+1)-th entries tie and sit in different lists (n_lists >= 2)
MERGE_EMPTY_QUERY = 6  # every list empty
MERGE_NQ = 7


def gen_merge_case(n_lists, k, seed=0, label_top=None):
    """[n_lists, MERGE_NQ, k] distances / labels.  Each list ascending by (distance, label), labels
    distinct over the whole case and >= 1, distances from {0..7} so that ties cross lists, fill levels
    from {0, 1, k // 2, k - 1, k} with -1 / FLT_MAX behind.  label_top: the largest label handed out."""
    rng = np.random.default_rng(1000 * n_lists + k + seed)
    nq = MERGE_NQ
    d = np.full((n_lists, nq, k), FLT_MAX, np.float32)
    l = np.full((n_lists, nq, k), -1, np.int32)
    total = n_lists * nq * k
    if label_top is None:
        pool = rng.permutation(np.arange(1, 4 * total + 1, dtype=np.int64))[:total]
    else:  # the top of the label range, 2^31 - 2 included
        pool = label_top - rng.permutation(np.arange(0, 4 * total, dtype=np.int64))[:total]
        pool[0] = label_top
        pool = rng.permutation(pool)
    pool = pool.reshape(n_lists, nq, k)
    fills = [0, 1, k // 2, k - 1, k]
    for q in range(nq):
        for i in range(n_lists):
            f = int(rng.choice(fills))
            if q == MERGE_EMPTY_QUERY:
                f = 0
            dd = rng.integers(0, 8, f).astype(np.float32)
            ll = pool[i, q, :f]
            if q == MERGE_TIE_QUERY and n_lists >= 2 and i < 2:
                # list 0: k - 1 zeros and one 5; list 1: a single 5 -- with the SMALLER label, so the
                # k-th slot goes to list 1's entry and list 0's 5 is the (k+1)-th
                f = k if i == 0 else 1
                dd = np.array([0.0] * (k - 1) + [5.0], np.float32) if i == 0 else np.array([5.0], np.float32)
                ll = np.sort(pool[i, q, :f])
            elif q == MERGE_TIE_QUERY and n_lists >= 2:
                dd = dd + np.float32(6.0)  # the other lists stay behind the cut
            o = np.lexsort((ll, dd))
            d[i, q, :f] = dd[o]
            l[i, q, :f] = ll[o]
        if q == MERGE_TIE_QUERY and n_lists >= 2:
            a, b = l[0, q, k - 1], l[1, q, 0]
            if a < b:  # make list 1's tied label the smaller one
                l[0, q, k - 1], l[1, q, 0] = b, a
    if label_top is not None:  # the largest label in use becomes label_top (it stays last in its run)
        l[l == l.max()] = label_top
    return d, l


def merge_cut_tie(d, l, k, q):
    """True when query q's k-th and (k+1)-th merged entries tie and come from different lists."""
    n_lists = d.shape[0]
    ent = [(d[i, q, j].view(np.uint32), int(l[i, q, j]), i) for i in range(n_lists) for j in range(d.shape[2])
           if l[i, q, j] >= 0]
    ent.sort()
    return len(ent) > k and ent[k - 1][0] == ent[k][0] and ent[k - 1][2] != ent[k][2]


REFINE_N = 3000
REFINE_NQ = 5


def gen_refine_case(D, R, seed=0):
    """Continuous data (gaussian x 30): Xq [5, D], Xt [3000, D], cand [5, R] distinct labels per query."""
    rng = np.random.default_rng(7000 + 31 * D + R + seed)
    Xt = (rng.normal(size=(REFINE_N, D)) * 30).astype(np.float32)
    Xq = (rng.normal(size=(REFINE_NQ, D)) * 30).astype(np.float32)
    cand = np.stack([rng.permutation(REFINE_N)[:R] for _ in range(REFINE_NQ)]).astype(np.int32)
    return Xq, Xt, cand


REFINE_DUP = (7, 100)     # Xt[100] == Xt[7]: an exact tie, the smaller label first
REFINE_TWICE = 11         # this label stands twice in query 1's list
REFINE_HUGE = 200         # a row of 1e20: the distance overflows
REFINE_NAN = 201          # a row holding a NaN
REFINE_EMPTY_QUERY = 3    # all candidates -1


def gen_refine_planted(D=128, R=257, seed=0):
    rng = np.random.default_rng(7100 + seed)
    Xq, Xt, cand = gen_refine_case(D, R, seed=seed + 1)
    for lab in (*REFINE_DUP, REFINE_TWICE, REFINE_HUGE, REFINE_NAN):  # planted by hand below
        cand[cand == lab] = 1 + lab  # (may repeat a neighbour's label: duplicates are legal)
    Xt[REFINE_DUP[0]] = Xq[0] + rng.normal(size=D).astype(np.float32)  # near query 0: both rank first
    Xt[REFINE_DUP[1]] = Xt[REFINE_DUP[0]]
    Xt[REFINE_TWICE] = Xq[1] + rng.normal(size=D).astype(np.float32)
    Xt[REFINE_HUGE] = np.float32(1e20)
    Xt[REFINE_NAN, D // 2] = np.nan
    cand[0, 5], cand[0, 2] = REFINE_DUP           # the larger label stands first in the list
    cand[1, 0] = cand[1, R - 1] = REFINE_TWICE
    cand[:, 1] = REFINE_HUGE
    cand[:, 3] = REFINE_NAN
    cand[REFINE_EMPTY_QUERY] = -1
    cand[4, 4::7] = -1                            # -1 scattered in the middle of a list
    cand[2, R // 2:] = -1                         # ... and as a tail
    return Xq, Xt, cand


def gen_encoder_planted(L, bits, seed=0):
    """Rows planted in PCA space for a codebook whose subspace 0 has 512 entries (two LDS chunks of
    256).  Returns (Xp, cents, rows) with rows = dict(name -> row index):
      nan       a NaN in sub-vector 0                    -> code 0 there
      inf       +inf in sub-vector 0                     -> code 0 there
      huge      1e20 everywhere: every distance is inf   -> code 0 everywhere
      negzero   -0.0 against the +0.0 centroid 5 of subspace 0
      dup       the row equals centroid 511 == centroid 0 of subspace 0: the first wins across chunks
    """
    assert bits[0] == 9
    rng = np.random.default_rng(8100 + L + seed)
    cents = [(rng.normal(size=(1 << b, L)) * 30).astype(np.float32) for b in bits]
    cents[0][5] = np.float32(0.0)
    cents[0][511] = cents[0][0]
    D = L * len(bits)
    Xp = (rng.normal(size=(40, D)) * 30).astype(np.float32)
    rows = dict(nan=3, inf=4, huge=5, negzero=6, dup=7)
    Xp[rows["nan"], L - 1] = np.nan
    Xp[rows["inf"], 0] = np.inf
    Xp[rows["huge"]] = np.float32(1e20)
    Xp[rows["negzero"], :L] = np.float32(-0.0)
    Xp[rows["dup"], :L] = cents[0][511]
    return Xp, cents, rows


def gen_project_input(n, D, seed=0):
    """gaussian x 30 with one NaN row (row 1 of n > 2, else none) and one row of 3e38 (the last)."""
    rng = np.random.default_rng(9000 + D + seed)
    X = (rng.normal(size=(n, D)) * 30).astype(np.float32)
    if n > 2:
        X[1, D // 2] = np.nan
    if n > 1:
        X[n - 1] = np.float32(3e38)
    return X


TIER_ROWS = 65537


def tier_ns(D, tier):
    """Row counts on both sides of launch_project's thresholds.  R = (256 / D) * 8 is the middle tier's rows
    per workgroup and divides 2048: n = 2049 leaves its last tile one row, n = 2048 + R - 1 leaves it R - 1."""
    return [2047, 2048, 2049, 2048 + (256 // D) * 8 - 1] if tier == "mid" else [65535, 65536, 65537]


def gen_tier_input(D):
    """65 537 rows of gaussian x 30; every n of tier_ns is a prefix (rows are independent).  Row 1 holds a
    NaN; row 2 and the LAST row of every prefix are 3e38 (sums that overflow)."""
    rng = np.random.default_rng(9000 + D)
    X = (rng.normal(size=(TIER_ROWS, D)) * 30).astype(np.float32)
    X[1, D // 2] = np.nan
    X[2] = np.float32(3e38)
    for n in tier_ns(D, "mid") + tier_ns(D, "big"):
        X[n - 1] = np.float32(3e38)
    return X


def rotation(D, seed=0, scale=1.0):
    q, _ = np.linalg.qr(np.random.default_rng(9500 + D + seed).normal(size=(D, D)))
    return (q * scale).astype(np.float32)


CHECKED_D = 64
CHECKED_NQ = 2048 + 5
CHECKED_INF_QUERY = 2050   # holds one +inf: inf * e is +-inf in every column, their sum NaN or inf
CHECKED_OVF_QUERY = 17     # 3e38 everywhere: the products with |e| > 1.14 overflow
CHECKED_ZERO_QUERY = 0     # the zero vector itself


def gen_checked_case(seed=0):
    """A sequential-sum index (one scalar quantiser per dimension) with D = 64 and mEigenVectors =
    16 x a rotation, so that 3e38 * e overflows IN THE PRODUCT for more than half of the entries and
    every coordinate of that query comes out non-finite (with a plain rotation, whose entries are
    below 1, no product of finite floats can overflow)."""
    rng = np.random.default_rng(9900 + seed)
    D, N = CHECKED_D, 1000
    bits = rng.integers(2, 5, D).tolist()
    cent = np.zeros((16, D), np.float32)
    for d, b in enumerate(bits):
        cent[: 1 << b, d] = np.sort(rng.normal(size=1 << b) * 480).astype(np.float32)
    codes = np.stack([rng.integers(0, 1 << b, N) for b in bits], 1).astype(np.uint16)
    eig = rotation(D, seed=seed, scale=16.0)
    X = (rng.normal(size=(CHECKED_NQ, D)) * 30).astype(np.float32)
    X[CHECKED_ZERO_QUERY] = 0.0
    X[CHECKED_INF_QUERY, 9] = np.inf
    X[CHECKED_OVF_QUERY] = np.float32(3e38)
    return dict(D=D, N=N, bits=bits, cent=cent, codes=codes, eig=eig, X=X)


def seq_all_dists(Xc, bits, cent, codes):
    """BitVecEngine::queryLUT's row distances for checked, projected queries Xc [nq, D]: per dimension
    lut = fl((x - c)^2), then ((l_0 + l_1) + l_2) + ... in float32.  [nq, N]."""
    nq = Xc.shape[0]
    acc = None
    for d, b in enumerate(bits):
        t = Xc[:, d:d + 1] - cent[None, : 1 << b, d]
        lut = (t * t).astype(np.float32)                # [nq, 1 << b]
        col = lut[:, codes[:, d].astype(np.int64)]      # [nq, N]
        acc = col if acc is None else (acc + col).astype(np.float32)
    assert acc.shape == (nq, codes.shape[0])
    return acc
