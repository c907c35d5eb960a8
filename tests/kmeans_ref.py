"""NumPy restatement of the k-means inside VAQ::clusterTI(true) -- KMeans::staticFitCodebook ->
staticFitSampling (KMeans.hpp:487-652, called at VAQ.cpp:896-900) -- and the inputs of the fixtures
under tests/golden/kmeans/ (regenerated here from a seed; the fixtures hold the reference's outputs
and a digest of these inputs).

Every float operation is a float32 operation in the reference's order:
  * squaredNorm of (x - mean) is Eigen's linear vectorised reduction (Eigen/src/Core/Redux.h,
    redux_impl<.., LinearVectorizedTraversal, NoUnrolling>) over 8-float packets with two accumulators,
    predux = ((a0+a4) + (a2+a6)) + ((a1+a5) + (a3+a7)), then the scalar tail; fewer than 8 columns:
    the plain sequential sum;
  * the comparison is made on sqrt(squaredNorm), strict, first minimum wins;
  * the new centre is (thread 0's sum + thread 1's sum) / float(count), each thread's sum taken in
    ascending row order from +0 (two OpenMP threads, static schedule).
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans")
MAX_ITER = 50            # VAQ.cpp:899
ROWS_PER_CENTRE = 256    # KMeans.hpp:619
SEED = 13517106          # utils/Random.hpp:18

# name: (N, seg, L, T, centroids per subspace, subspaces of the index)
CASES = {
    "n3000_s2_l8_t16": (3000, 2, 8, 16, 16, 4),         # unsampled, dimen 16 (two packets), converges
    "n70000_s2_l16_t64": (70000, 2, 16, 64, 256, 8),    # sampled (16384 rows), dimen 32; byte-code layout
    "n5000_s3_l4_t37": (5000, 3, 4, 37, 8, 4),          # dimen 12: one packet and a scalar tail
    "n20000_s1_l20_t50": (20000, 1, 20, 50, 32, 4),     # sampled, dimen 20, empty clusters: runs to the cap
    "n40000_s4_l16_t100": (40000, 4, 16, 100, 256, 4),  # dimen 64: the unrolled loop runs; decides the order
    "n4001_s5_l8_t24": (4001, 5, 8, 24, 16, 8),         # odd row count (halves of 2001 / 2000), dimen 40: odd packet
    "n2500_s1_l6_t10": (2500, 1, 6, 10, 64, 4),         # dimen 6: no packet at all
    "n301_s4_l128_t7": (301, 4, 128, 7, 4, 4),          # dimen 512: decoded rows too wide for a workgroup's LDS tile
}


def make_inputs(name: str):
    """(codes N x M uint16, [M codebooks ncent x L float32]) of a case, from its fixed seed."""
    N, seg, L, T, ncent, M = CASES[name]
    rng = np.random.default_rng(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    cents = [rng.normal(size=(ncent, L)).astype(np.float32) for _ in range(M)]
    codes = rng.integers(0, ncent, size=(N, M), dtype=np.int64).astype(np.uint16)
    return codes, cents


def digest(codes, cents) -> str:
    h = hashlib.sha256()
    for a in [codes] + list(cents):
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def load_fixture(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def permutation_head(n: int, r: int, seed: int = SEED) -> np.ndarray:
    """The first r entries of randomPermutation(n) (utils/Random.hpp:18-28): entry i is final after
    step i, so r steps over a sparse map of the touched positions suffice."""
    r = min(r, n)
    steps = min(r, max(n - 1, 0))
    rs = np.random.RandomState(seed)  # init_genrand(seed): the std::mt19937(seed) state
    raw = rs._bit_generator.random_raw(steps) if steps else np.empty(0, np.uint64)
    moved = {}
    out = np.empty(r, np.int64)
    for i in range(steps):
        i2 = i + int(raw[i]) % (n - i)
        vi, v2 = moved.get(i, i), moved.get(i2, i2)
        moved[i2] = vi
        out[i] = v2
    for i in range(steps, r):
        out[i] = moved.get(i, i)
    return out


def decode(codes, cents, rows, seg) -> np.ndarray:
    cb = np.asarray(codes)[rows]
    return np.ascontiguousarray(np.concatenate(
        [np.asarray(cents[s], np.float32)[cb[:, s].astype(np.int64)] for s in range(seg)], axis=1))


def sqnorm_eigen(sq: np.ndarray) -> np.ndarray:
    """Eigen's sum over the last axis of the float32 array sq (the squared differences)."""
    d = sq.shape[-1]
    if d < 8:
        res = sq[..., 0].copy()
        for j in range(1, d):
            res = res + sq[..., j]
        return res
    p = d // 8
    end2 = (d // 16) * 16
    a0 = sq[..., 0:8].copy()
    if p > 1:
        a1 = sq[..., 8:16].copy()
        for i in range(16, end2, 16):
            a0 = a0 + sq[..., i:i + 8]
            a1 = a1 + sq[..., i + 8:i + 16]
        a0 = a0 + a1
        if p * 8 > end2:
            a0 = a0 + sq[..., end2:end2 + 8]
    b = a0[..., 0:4] + a0[..., 4:8]
    res = (b[..., 0] + b[..., 2]) + (b[..., 1] + b[..., 3])
    for j in range(p * 8, d):
        res = res + sq[..., j]
    return res


def sqnorm_sequential(sq: np.ndarray) -> np.ndarray:
    """res = 0; res += t * t column by column (the order the encoder's distances use)."""
    res = np.zeros(sq.shape[:-1], np.float32)
    for j in range(sq.shape[-1]):
        res = res + sq[..., j]
    return res


def _reduce(order):
    return sqnorm_eigen if order == "eigen" else sqnorm_sequential


def assign_full(X, means, order="eigen", chunk=1 << 22):
    """belongs_to[i]: first j with the smallest sqrt(|X[i] - means[j]|^2) below FLT_MAX, -1 if none."""
    n, d = X.shape
    T = means.shape[0]
    red = _reduce(order)
    out = np.empty(n, np.int64)
    step = max(1, chunk // (T * d))
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, n, step):
            diff = X[r0:r0 + step, None, :] - means[None, :, :]
            dist = np.sqrt(red(diff * diff))
            assert dist.dtype == np.float32
            # strict `<` against a running minimum that starts at FLT_MAX; NaN never wins
            dist = np.where(dist < np.finfo(np.float32).max, dist, np.float32(np.inf))
            j = np.argmin(dist, axis=1)  # first minimum
            out[r0:r0 + step] = np.where(np.isinf(dist[np.arange(len(j)), j]), -1, j)
    return out


def assign(X, means, order="eigen"):
    """assign_full, with the float32 distance evaluated only where it can matter: a float64 estimate of the
    squared distance rules out every centre more than 1e-3 (relative) above the row's smallest -- the float32
    sum of d <= 1024 squares is within (d + 2) * 2^-24 < 7e-5 of the exact value, whatever its order."""
    n, d = X.shape
    finite = np.nonzero(~np.isnan(means).any(axis=1))[0]
    if len(finite) == 0 or not np.isfinite(X).all() or not np.isfinite(means[finite]).all() or \
            max(np.abs(X).max(), np.abs(means[finite]).max()) > 1e15:
        return assign_full(X, means, order)
    X64, m64 = X.astype(np.float64), means[finite].astype(np.float64)
    est = (X64 * X64).sum(1)[:, None] - 2.0 * (X64 @ m64.T) + (m64 * m64).sum(1)[None, :]
    scale = (X64 * X64).sum(1) + (m64 * m64).sum(1).max()
    lo = est.min(axis=1)
    pi, pj = np.nonzero(est <= (lo + 1e-3 * np.abs(lo) + 1e-9 * scale)[:, None])
    pj = finite[pj]
    diff = X[pi] - means[pj]
    dist = np.sqrt(_reduce(order)(diff * diff))
    assert dist.dtype == np.float32 and (dist < np.finfo(np.float32).max).all()
    o = np.lexsort((pj, dist, pi))  # by row, then distance, then centre: the first of a row is its answer
    first = np.ones(len(o), bool)
    first[1:] = pi[o][1:] != pi[o][:-1]
    out = np.full(n, -1, np.int64)
    out[pi[o][first]] = pj[o][first]
    return out


def _ordered_sum(rows: np.ndarray) -> np.ndarray:
    """float32 sum of the rows from +0 in order (np.add.accumulate is sequential)."""
    z = np.zeros((1, rows.shape[1]), np.float32)
    return np.add.accumulate(np.concatenate([z, rows]), axis=0, dtype=np.float32)[-1]


def fit(X: np.ndarray, T: int, max_iter: int = MAX_ITER, order="eigen"):
    """staticFitSampling on the rows X (KMeans.hpp:509-615): (means, iterations)."""
    X = np.ascontiguousarray(X, np.float32)
    n, d = X.shape
    assert T <= n, "the reference reads out of bounds"
    means = X[permutation_head(n, T)].copy()
    half = (n + 1) // 2  # schedule(static), two threads
    changed, it = True, 0
    while changed and it < max_iter:
        b = assign(X, means, order)
        assert (b >= 0).all(), "the reference would index row -1"
        new = np.empty_like(means)
        with np.errstate(invalid="ignore", divide="ignore"):
            for c in range(T):
                m = np.nonzero(b == c)[0]
                p0 = _ordered_sum(X[m[m < half]])
                p1 = _ordered_sum(X[m[m >= half]])
                new[c] = ((np.float32(0) + p0) + p1) / np.float32(len(m))
        changed = False
        for c in range(T):
            if not np.array_equal(new[c], means[c]):  # elementwise ==: NaN is never equal
                changed = True
                means[c] = new[c]
        it += 1
    return means, it


def sample_rows(N: int, T: int) -> np.ndarray:
    """Rows staticFitCodebook works on (KMeans.hpp:626-647), in its order."""
    if N > ROWS_PER_CENTRE * T:
        return permutation_head(N, ROWS_PER_CENTRE * T)
    return np.arange(N, dtype=np.int64)


def fit_codebook(codes, cents, seg: int, T: int, max_iter: int = MAX_ITER, order="eigen"):
    """KMeans::staticFitCodebook: (means T x seg*L, iterations, NaN row mask)."""
    X = decode(codes, cents, sample_rows(len(codes), T), seg)
    means, it = fit(X, T, max_iter, order)
    return means, it, np.isnan(means).any(axis=1)


def assert_centres_equal(got, want, what=""):
    """Bit patterns where finite; NaN by position (its sign and payload are the machine's)."""
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ ({gn.sum()} vs {wn.sum()})"
    gb = np.where(gn, 0, got.view(np.uint32))
    wb = np.where(wn, 0, want.view(np.uint32))
    bad = gb != wb
    assert not bad.any(), f"{what}: {bad.sum()} values differ in {np.unique(np.nonzero(bad)[0]).size} centres"
