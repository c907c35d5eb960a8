"""NumPy oracle of the hierarchical codebook fit (vaqhip_fit_codebooks_hier; VAQ::train with mHierarchicalKmeans,
VAQ.cpp:535-594), composed of the pinned restatements and nothing else: kmeans_ref.permutation_head (randomPermutation),
kmeans_ref.fit (KMeans::staticFitSampling's Lloyd loop), kmeans_ref.sqnorm_eigen (Eigen's squaredNorm),
primitives_ref.argmin_strict (the encoder's strict argmin, no sqrt) and codebooks_ref.fit_codebooks for the flat
subspaces.  VAQ.cpp does not compile, so there is no recorded fixture: this composition is the reference.
"""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import codebooks_ref as cr
import kmeans_ref as kr
import primitives_ref as pr

K1 = 128
FLAT_MAX_BITS = 8
FLT_MAX = np.finfo(np.float32).max

# name: (n, D, M, bits, kind, salt).  kind: "float" blobs, "rotated" the same behind a random orthogonal eigvec,
# "paired" blobs whose last third of the rows repeats the first third (equal rows: stage-2 seeds that coincide leave an empty
# cluster, a NaN centre, and that fit runs to max_iter), "planted" blobs of equal size in which the row that seeds
# stage-1 centre i lies in blob i (so the groups are the blobs: 31 or 32 rows for 8 centres).  salt: part of the seed,
# chosen so that the case is a valid input -- Lloyd from random seeds leaves an empty or tiny stage-1 cluster on most
# draws of this size -- (tests/test_codebooks_hier_cpu.py asserts the conditions).
CASES = {
    "tiny": (3000, 4, 2, (9, 3), "float", 2),
    "l12": (4001, 12, 1, (10,), "planted", 0),
    "two": (6000, 16, 4, (10, 9, 8, 5), "rotated", 33),
    "resampled": (70000, 2, 1, (9,), "float", 2),
    "resampled2": (70000, 2, 2, (9, 9), "float", 0),  # two subspaces whose stage 1 samples for itself, in one call
    "budget": (20000, 4, 2, (9, 11), "paired", 2),
}
BLOBS = 128     # blobs of a hierarchical subspace, far apart; the noise is uniform (no stray row to hold a centre alone)
SPREAD = 24.0
NOISE = 0.5


def hierarchical(b: int) -> bool:
    return b > FLAT_MAX_BITS


def rows_for(n: int, b: int, B: int, M: int) -> int:
    """VAQ.cpp:535-536"""
    return min(n, max(256 << b, 256 << (B // M)))


def group_limit(K2: int) -> int:
    return max(256 * K2, 65536)


def stage1_seed_rows(n: int, b: int, B: int, M: int):
    """rows of the input matrix that seed the 128 stage-1 centres of a b-bit subspace"""
    rows = rows_for(n, b, B, M)
    work = cr.sample_count(rows, K1)
    seeds = kr.permutation_head(work, K1)
    if work < rows:
        seeds = kr.permutation_head(rows, work)[seeds]
    return kr.permutation_head(n, rows)[seeds]


def make_inputs(name: str):
    """(X n x D float32, eigvec or None) of a case, from its fixed seed."""
    n, D, M, bits, kind, salt = CASES[name]
    rng = np.random.default_rng(int(hashlib.sha256(("codebooks_hier:%s:%d" % (name, salt)).encode()).hexdigest()[:8], 16))
    L = D // M
    X = np.empty((n, D), np.float32)
    for s in range(M):
        nb = BLOBS if hierarchical(bits[s]) else 1 << bits[s]
        blobs = (rng.normal(size=(nb, L)) * SPREAD).astype(np.float32)
        label = rng.integers(0, nb, n)
        if kind == "planted" and hierarchical(bits[s]):
            label = rng.permutation(np.arange(n) % nb)
            label[stage1_seed_rows(n, bits[s], sum(bits), M)] = np.arange(K1)
        X[:, s * L:(s + 1) * L] = blobs[label] + (rng.uniform(-NOISE, NOISE, size=(n, L))).astype(np.float32)
    if kind == "paired":
        X[n - n // 3:] = X[:n // 3]
    if kind != "rotated":
        return X, None
    q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    eig = np.ascontiguousarray(q, np.float32)
    return np.ascontiguousarray(X @ eig.T, np.float32), eig


def sq_dist_eigen(Xs, C, chunk=1 << 22):
    """[rows, centres] float32: (x - c).squaredNorm() in Eigen's order."""
    Xs = np.ascontiguousarray(Xs, np.float32)
    C = np.ascontiguousarray(C, np.float32)
    out = np.empty((len(Xs), len(C)), np.float32)
    step = max(1, chunk // (C.shape[0] * C.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, len(Xs), step):
            diff = Xs[r0:r0 + step, None, :] - C[None, :, :]
            out[r0:r0 + step] = kr.sqnorm_eigen(diff * diff)
    assert out.dtype == np.float32
    return out


def membership(Xs, C):
    """(group of every row, rows without any centre): the nearest centre by squaredNorm, NO sqrt, centres ascending,
    strict < against FLT_MAX -- the encoder's rule."""
    d2 = sq_dist_eigen(Xs, C)
    return pr.argmin_strict(d2).astype(np.int64), ~(d2 < FLT_MAX).any(axis=1)


def fit_subspace_hier(Rs, bits_s: int, max_iter: int):
    """One hierarchical subspace from its rows R_s (rows_s x L): a dict with the k_s x L centres, the largest iteration
    count of the 129 fits, and what the valid-input conditions are checked on (C1, group sizes, per-fit iterations)."""
    K2 = 1 << (bits_s - 7)
    rows = len(Rs)
    work = cr.sample_count(rows, K1)  # staticFitSampling samples for itself
    R1 = Rs[kr.permutation_head(rows, work)] if work < rows else Rs
    C1, it1 = kr.fit(R1, K1, max_iter)
    g, lost = membership(Rs, C1)
    sizes = np.bincount(g, minlength=K1)
    out = dict(C1=C1, it1=it1, sizes=sizes, lost=int(lost.sum()), K2=K2, it2=[], centres=None)
    if np.isnan(C1).any() or lost.any() or (sizes < K2).any() or (sizes > group_limit(K2)).any():
        return out  # refused by the library
    cents = np.empty((K1 * K2, Rs.shape[1]), np.float32)
    for i in range(K1):
        cents[i * K2:(i + 1) * K2], it = kr.fit(Rs[g == i], K2, max_iter)  # (boolean mask: ascending position in R_s)
        out["it2"].append(it)
    out["centres"] = cents
    out["iters"] = max([it1] + out["it2"])
    return out


def fit_codebooks_hier(X, M, bits, eig=None, max_iter: int = cr.MAX_ITER):
    """([M centre matrices], [iterations], [NaN-row masks], {s: details of hierarchical subspace s}); a centre matrix is
    None where the library refuses the subspace."""
    n, D = X.shape
    L = D // M
    if not any(hierarchical(b) for b in bits):
        return cr.fit_codebooks(X, M, bits, eig, max_iter) + ({},)
    # the flat subspaces: a subspace's fit does not depend on its neighbours' bits
    flat_bits = [b if not hierarchical(b) else 1 for b in bits]
    cents, iters, nans = cr.fit_codebooks(X, M, flat_bits, eig, max_iter)
    B = sum(bits)
    rows = {s: rows_for(n, bits[s], B, M) for s in range(M) if hierarchical(bits[s])}
    head = kr.permutation_head(n, max(rows.values()))
    R = cr.projected_rows(X[head], eig)  # (a row's projection is its own)
    info = {}
    for s, rs in rows.items():
        assert rs >= 1 << bits[s], "refused before any device work"
        d = fit_subspace_hier(np.ascontiguousarray(R[:rs, s * L:(s + 1) * L]), bits[s], max_iter)
        info[s] = d
        cents[s] = d["centres"]
        iters[s] = d.get("iters", 0)
        nans[s] = np.isnan(d["centres"]).any(axis=1) if d["centres"] is not None else None
    return cents, iters, nans, info


@functools.lru_cache(maxsize=None)
def inputs(name):
    return make_inputs(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's answer for a case, computed once per process"""
    n, D, M, bits, kind, salt = CASES[name]
    X, eig = inputs(name)
    return fit_codebooks_hier(X, M, bits, eig)


BYTES_SEED = 0  # chosen like a salt: the byte rows below are a valid input


@functools.lru_cache(maxsize=None)
def byte_inputs():
    """(uint8 rows with values 0..255 of `two`'s shape, `two`'s eigvec)"""
    n, D, M, bits, kind, salt = CASES["two"]
    rng = np.random.default_rng(int(hashlib.sha256(("codebooks_hier:bytes:%d" % BYTES_SEED).encode()).hexdigest()[:8], 16))
    return rng.integers(0, 256, size=(n, D), dtype=np.int64).astype(np.uint8), inputs("two")[1]


@functools.lru_cache(maxsize=None)
def expected_bytes():
    n, D, M, bits, kind, salt = CASES["two"]
    X8, eig = byte_inputs()
    return fit_codebooks_hier(X8.astype(np.float32), M, bits, eig)
