"""The two lambdas of BitVecEngine::binaryEncodingLUT restated in numpy: centroidsQuantile
(BitVecEngine.hpp:811-840) and encodeToLUTCode (:889-932), and the case tables the CPU and GPU tests of
the GPU build (vaq_amd/csrc/vaq_lutfit.h, vaq_lutfit.hip) share.

float32 scalars throughout; double exactly where the reference has it (the 0.5 literals of :818).  A bucket's
sum is a sequential float32 accumulate from +0 (centroids[i] += Z[lastidx] on the 0 of setZero()).

Not pinned against a compiled reference: BitVecEngine.hpp includes glpk.h."""
import functools
import math

import numpy as np

F = np.float32
MAX_CENT = 256
MAX_Q = 257


def float_to_key(a):
    u = np.ascontiguousarray(a, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F)


def sort_column(col):
    """std::sort(sortedVec) -- ascending; -0 before +0 (std::sort leaves the two in an order of its own: they
    compare equal there, so nothing but the sign of a zero quantile can tell)."""
    return key_to_float(np.sort(float_to_key(col)))


def quantile_pos(i, N, n):
    p = F(i + 1) / F(N)                                                   # (float)(i+1)/N
    return F(float(F(1) - p) * (-0.5) + float(p) * (float(F(n)) - 0.5))  # double, rounded by `float poi =`


def centroids_quantile(Z, N):
    """Z sorted ascending (float32).  Returns (Q [N + 1], centroids [N])."""
    n = Z.shape[0]
    Q = np.zeros(N + 1, F)
    Q[0] = Z[0]
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(N - 1):
            poi = quantile_pos(i, N, n)
            left = max(int(math.floor(poi)), 0)
            right = min(int(math.ceil(poi)), n - 1)
            f = F(poi - F(left))
            Q[i + 1] = F(F(F(1) - f) * Z[left]) + F(f * Z[right])
        Q[N] = Z[-1]
        cent = np.zeros(N, F)
        zl = Z.tolist()  # float32 values as doubles: <= compares the same
        lastidx = 0
        for i in range(N):
            q = float(Q[i + 1])
            first = lastidx
            while lastidx < n and zl[lastidx] <= q:
                lastidx += 1
            count = lastidx - first
            if count > 0:
                s = np.cumsum(np.concatenate([np.zeros(1, F), Z[first:lastidx]]), dtype=F)[-1]
                cent[i] = F(s) / F(count)
            else:
                cent[i] = F(Q[i] + Q[i + 1]) / F(2.0)
    return Q, cent


def fit(X, bits):
    """X n x D in PCA space.  Returns (centroidsMat 256 x D, Q D x 257), zero where the reference has no entry."""
    X = np.ascontiguousarray(X, F)
    D = X.shape[1]
    cent = np.zeros((MAX_CENT, D), F)
    Qs = np.zeros((D, MAX_Q), F)
    for d, b in enumerate(bits):
        N = 1 << b
        Q, c = centroids_quantile(sort_column(X[:, d]), N)
        Qs[d, :N + 1] = Q
        cent[:N, d] = c
    return cent, Qs


def encode_column(x, Q, c, N):
    """encodeToLUTCode for one dimension: x [n] float32, Q [N + 1], c [N].  uint16 codes."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore"):
        le = x[:, None] <= Q[None, :N + 1]
        found = le.any(axis=1)
        q = np.where(found, le.argmax(axis=1), N + 1)  # the first q with x <= Q[q]

        def dist(idx):
            return np.abs((x - c[np.clip(idx, 0, N - 1)]).astype(F))
        m, l, r = dist(q - 1), dist(q - 2), dist(q)
        mid = np.where((m <= l) & (m <= r), q - 1, np.where((l <= m) & (l <= r), q - 2, q))
        code = np.where(~found, N - 1,
               np.where(q == 0, 0,
               np.where(q == 1, np.where(m <= r, 0, 1),
               np.where(q == N, np.where(m <= l, N - 1, N - 2), mid))))
    return code.astype(np.uint8).astype(np.uint16)  # (uint8_t)code, :924


def encode(Xp, bits, cent, Qs):
    Xp = np.ascontiguousarray(Xp, F)
    return np.stack([encode_column(Xp[:, d], Qs[d], cent[:, d], 1 << b) for d, b in enumerate(bits)], 1)


def first_argmin(x, c, N):
    """vaqhip_encode's rule on a scalar quantiser: the first global argmin under strict <"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(x, F)[:, None] - c[None, :N]).astype(F)
        return (d * d).astype(F).argmin(axis=1)


# ---- case tables ----
def _rng(name):
    return np.random.default_rng(abs(hash_name(name)))


def hash_name(name):
    import hashlib
    return int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)


FIT_CASES = ("n1", "n3_b8", "n4099_d5", "const", "grid", "n70001_b1")


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """(X n x D float32 in PCA space, bits)"""
    rng = _rng(name)
    if name == "n1":  # a single training row
        return np.array([[1.5, -2.25, 0.0]], F), [1, 3, 8]
    if name == "n3_b8":  # n < N: almost every bucket empty
        return (rng.normal(size=(3, 2)) * 5).astype(F), [8, 2]
    if name == "n4099_d5":  # D not a multiple of 4, n not a multiple of 64
        return (rng.normal(size=(4099, 5)) * np.array([20, 9, 4, 2, 1])).astype(F), [8, 5, 3, 2, 1]
    if name == "const":  # all Q equal up to the rounding of the interpolation
        X = np.empty((1000, 4), F)
        X[:] = np.array([3.7, 0.0, -1e-3, 1e30], F)
        return X, [4, 8, 1, 6]
    if name == "grid":  # heavy duplicates: empty buckets, integer centres, m == r and m == l ties
        X = rng.integers(-3, 4, size=(5000, 4)).astype(F)
        X[:, 3] = rng.integers(0, 2, size=5000) * 2  # two values only
        X[::7, 1] = -0.0
        return X, [8, 4, 2, 1]
    if name == "n70001_b1":  # one bucket longer than any LDS stage
        return (rng.normal(size=(70001, 2)) * 3).astype(F), [1, 3]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def fit_ref(name):
    X, bits = fit_case(name)
    return fit(X, bits)


@functools.lru_cache(maxsize=None)
def probes(name):
    """Rows to encode under the fit of a case: every Q[q] itself, the value midway between neighbouring centres,
    values below Q[0] and above Q[N], the neighbours of every boundary, NaN and +-inf, and training rows."""
    X, bits = fit_case(name)
    cent, Qs = fit_ref(name)
    cols = []
    with np.errstate(over="ignore", invalid="ignore"):
        for d, b in enumerate(bits):
            N = 1 << b
            Q, c = Qs[d, :N + 1], cent[:N, d]
            mid = ((c[:-1] + c[1:]) / F(2)).astype(F)
            v = np.concatenate([Q, mid, np.nextafter(Q, F(np.inf)), np.nextafter(Q, F(-np.inf)), c,
                                np.array([Q[0] - F(1), Q[0] - F(1e6), Q[N] + F(1), Q[N] + F(1e6), np.nan, np.inf, -np.inf,
                                          0.0, -0.0, 3.4e38, -3.4e38], F),
                                X[:200, d]]).astype(F)
            cols.append(v)
    m = max(len(v) for v in cols)
    return np.stack([np.resize(v, m) for v in cols], 1).astype(F)


@functools.lru_cache(maxsize=None)
def codes_ref(name):
    _, bits = fit_case(name)
    cent, Qs = fit_ref(name)
    return encode(probes(name), bits, cent, Qs)
