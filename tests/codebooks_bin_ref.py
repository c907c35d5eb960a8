"""NumPy oracle of the binary-tree codebook fit (vaqhip_fit_codebooks_bin; VAQ::train with mBinaryKmeans,
hierarchicalBinKmeans, VAQ.cpp:1293-1371), composed of the pinned restatements and nothing else:
kmeans_ref.permutation_head (randomPermutation), kmeans_ref.fit (KMeans::staticFitSampling's Lloyd loop),
kmeans_ref.sqnorm_eigen (Eigen's squaredNorm), codebooks_ref.fit_codebooks for the flat subspaces,
codebooks_ref.projected_rows, and the hierarchical form's rows_for.  VAQ.cpp does not compile, so there is no recorded
fixture: this composition is the reference (parity-unpinned in the sense of DESIGN.md section 2, like
tests/codebooks_hier_ref.py).
"""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import codebooks_ref as cr
import kmeans_ref as kr
from codebooks_hier_ref import rows_for

FLAT_MAX_BITS = 8
LEAF, CUT, SPLIT = "leaf", "cut", "split"

# name: (n, D, M, bits, kind, salt).  kind: "float" blobs, "rotated" the same behind a random orthogonal eigvec, "paired"
# blobs whose last third of the rows repeats the first third (equal rows: two seeds that coincide leave an empty cluster,
# a NaN centre), "far" blobs with 100 rows far from the rest (the root's 2-centre fit isolates them: fewer than 256),
# "skew" three quarters of the rows in one distant region (the root and that child hold more than 65536 rows),
# "skewfar" a tight region of 70% of the rows with 100 rows far from it, and a distant region with the rest (the root
# splits the regions, the large child isolates the 100 and is cut with more than 65536 rows).
# (With M = 1 and 9 bits rows_s = 131072 = 256 * 512, so a cut AT the root never samples; the cut fit that samples is
# the depth-2 node's: 256 centres over more than 65536 rows.)
# salt: part of the seed, chosen on the CPU so that the case shows what its row names
# (tests/test_codebooks_bin_cpu.py asserts it from the tree).
CASES = {
    "tiny": (3000, 4, 2, (9, 3), "float", 0),
    "l1": (3000, 2, 2, (9, 9), "float", 0),
    "l12": (4001, 12, 1, (10,), "float", 0),
    "wide": (2500, 65, 1, (9,), "float", 0),
    "two": (6000, 16, 4, (10, 9, 8, 5), "rotated", 0),
    "paired": (20000, 4, 2, (9, 11), "paired", 0),
    "rootcut": (3000, 2, 1, (9,), "far", 0),
    "resampled": (140000, 2, 1, (9,), "skew", 0),
    "cutsampled": (140000, 2, 1, (9,), "skewfar", 0),
}
BLOBS = 128
SPREAD = 24.0
NOISE = 0.5


def binary(b: int) -> bool:
    return b > FLAT_MAX_BITS


def make_inputs(name: str):
    """(X n x D float32, eigvec or None) of a case, from its fixed seed."""
    n, D, M, bits, kind, salt = CASES[name]
    rng = np.random.default_rng(int(hashlib.sha256(("codebooks_bin:%s:%d" % (name, salt)).encode()).hexdigest()[:8], 16))
    L = D // M
    X = np.empty((n, D), np.float32)
    for s in range(M):
        nb = BLOBS if binary(bits[s]) else 1 << bits[s]
        blobs = (rng.normal(size=(nb, L)) * SPREAD).astype(np.float32)
        label = rng.integers(0, nb, n)
        V = blobs[label] + (rng.uniform(-NOISE, NOISE, size=(n, L))).astype(np.float32)
        if kind == "far" and binary(bits[s]):
            V[rng.choice(n, 100, replace=False)] += np.float32(1.0e5)
        if kind == "skew" and binary(bits[s]):
            V[label < nb // 4] += np.float32(5000.0)
        if kind == "skewfar" and binary(bits[s]):
            tight = rng.uniform(size=n) < 0.7
            V[~tight] += np.float32(10000.0)
            V[tight] = (rng.uniform(-4.0, 4.0, size=(int(tight.sum()), L))).astype(np.float32)
            far = rng.choice(np.nonzero(tight)[0], 100, replace=False)
            V[far] -= np.float32(8000.0)
        X[:, s * L:(s + 1) * L] = V
    if kind == "paired":
        X[n - n // 3:] = X[:n // 3]
    if kind != "rotated":
        return X, None
    q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    eig = np.ascontiguousarray(q, np.float32)
    return np.ascontiguousarray(X @ eig.T, np.float32), eig


def sq_dist_eigen(Xs, C):
    """[rows, centres] float32: (x - c).squaredNorm() in Eigen's order (sequential below 8 columns)."""
    Xs = np.ascontiguousarray(Xs, np.float32)
    C = np.ascontiguousarray(C, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = Xs[:, None, :] - C[None, :, :]
        out = kr.sqnorm_eigen(diff * diff)
    assert out.dtype == np.float32
    return out


def goes_left(Xs, C):
    """getBelongsToBinaryCluster (VAQ.cpp:1293-1310): left iff left < right on the squaredNorms themselves, NO sqrt; a tie
    and a NaN on either side go right."""
    d2 = sq_dist_eigen(Xs, C[:2])
    with np.errstate(invalid="ignore"):
        return d2[:, 0] < d2[:, 1]


def fit_sampling(Xs, k: int, max_iter: int):
    """staticFitSampling as it behaves when handed the rows Xs: (means, iterations, sampled?)"""
    m = len(Xs)
    work = cr.sample_count(m, k)
    if work < m:
        Xs = Xs[kr.permutation_head(m, work)]
    means, it = kr.fit(Xs, k, max_iter)
    return means, it, work < m


def fit_subspace_bin(Rs, bits_s: int, max_iter: int):
    """One binary subspace from its rows R_s (rows_s x L): (k_s x L centres, tree).  tree: one dict per node in level
    order -- depth, index, rows, sizeleft, sizeright (None for a leaf), kind, iters (the 2-centre fit's), sampled (that
    fit), nan2 (a NaN among its two centres), and for a cut node cut_iters, cut_sampled."""
    k = 1 << bits_s
    cents = np.full((k, Rs.shape[1]), np.float32(-12345.0), np.float32)
    tree = []
    level = [(0, np.arange(len(Rs)))]
    for d in range(1, bits_s + 1):
        tempK = 1 << (bits_s - d + 1)
        nxt = []
        for j, rows in level:
            X = Rs[rows]
            assert len(X) >= tempK
            C, it, sampled = fit_sampling(X, 2, max_iter)
            node = dict(depth=d, index=j, rows=len(rows), sizeleft=None, sizeright=None, kind=LEAF, iters=it, sampled=sampled,
                        nan2=bool(np.isnan(C).any()))
            tree.append(node)
            if d == bits_s:
                cents[j * tempK:(j + 1) * tempK] = C
                continue
            left = goes_left(X, C)
            node["sizeleft"], node["sizeright"] = int(left.sum()), int((~left).sum())
            if node["sizeleft"] < tempK // 2 or node["sizeright"] < tempK // 2:
                node["kind"] = CUT
                cents[j * tempK:(j + 1) * tempK], node["cut_iters"], node["cut_sampled"] = fit_sampling(X, tempK, max_iter)
                continue
            node["kind"] = SPLIT
            nxt.append((2 * j, rows[left]))      # (boolean masks: ascending position within the node)
            nxt.append((2 * j + 1, rows[~left]))
        level = nxt
        if not level:
            break
    return cents, tree


def tree_stats(trees):
    """the figures vaqhip_last_fit_codebooks_bin_timing reports, from the trees of a call's binary subspaces"""
    nodes = [nd for t in trees for nd in t]
    leaves = [nd["rows"] for nd in nodes if nd["kind"] == LEAF]
    return dict(levels=max(nd["depth"] for nd in nodes), nodes=len(nodes),
                cut_nodes=sum(nd["kind"] == CUT for nd in nodes), leaf_nodes=len(leaves),
                resampled_fits=sum(nd["sampled"] for nd in nodes) + sum(nd.get("cut_sampled", False) for nd in nodes),
                min_leaf_rows=min(leaves, default=0), max_leaf_rows=max(leaves, default=0))


def fit_codebooks_bin(X, M, bits, eig=None, max_iter: int = cr.MAX_ITER):
    """([M centre matrices], [iterations], [NaN-row masks], {s: tree of binary subspace s})"""
    n, D = X.shape
    L = D // M
    if not any(binary(b) for b in bits):
        return cr.fit_codebooks(X, M, bits, eig, max_iter) + ({},)
    flat_bits = [b if not binary(b) else 1 for b in bits]  # (a subspace's fit does not depend on its neighbours' bits)
    cents, iters, nans = cr.fit_codebooks(X, M, flat_bits, eig, max_iter)
    B = sum(bits)
    rows = {s: rows_for(n, bits[s], B, M) for s in range(M) if binary(bits[s])}
    head = kr.permutation_head(n, max(rows.values()))
    R = cr.projected_rows(X[head], eig)  # (a row's projection is its own)
    trees = {}
    for s, rs in rows.items():
        assert rs >= 1 << bits[s], "refused before any device work"
        cents[s], trees[s] = fit_subspace_bin(np.ascontiguousarray(R[:rs, s * L:(s + 1) * L]), bits[s], max_iter)
        iters[s] = max(max(nd["iters"], nd.get("cut_iters", 0)) for nd in trees[s])
        nans[s] = np.isnan(cents[s]).any(axis=1)
    return cents, iters, nans, trees


@functools.lru_cache(maxsize=None)
def inputs(name):
    return make_inputs(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's answer for a case, computed once per process"""
    n, D, M, bits, kind, salt = CASES[name]
    X, eig = inputs(name)
    return fit_codebooks_bin(X, M, bits, eig)


@functools.lru_cache(maxsize=None)
def byte_inputs():
    """(uint8 rows with values 0..255 of `two`'s shape, `two`'s eigvec)"""
    n, D, M, bits, kind, salt = CASES["two"]
    rng = np.random.default_rng(int(hashlib.sha256(b"codebooks_bin:bytes:0").hexdigest()[:8], 16))
    return rng.integers(0, 256, size=(n, D), dtype=np.int64).astype(np.uint8), inputs("two")[1]


@functools.lru_cache(maxsize=None)
def expected_bytes():
    n, D, M, bits, kind, salt = CASES["two"]
    X8, eig = byte_inputs()
    return fit_codebooks_bin(X8.astype(np.float32), M, bits, eig)
