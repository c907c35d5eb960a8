"""NumPy / plain Python restatement of the Hamming half of BitVecEngine, the checker of tests/test_bitvec_*.py.
tests/golden/hamming/ pins it to the compiled reference's KNNFromDists (README.md there).

  hamming_dists                      utils/DistanceFunctions.hpp:164-172 over all words, nothing masked
  query_sort                         BitVecEngine.cpp:60-76 (hammingDist, then KNNFromDists: fast_ref.knn_from_dists)
  std_sort_perm_f32                  libstdc++ std::sort of (idx, float dist) pairs under a distance-only comparator
  knn_from_dists_indices_supplied    BitVecEngine.hpp:171-187
  euclidean_no_sqrt                  utils/DistanceFunctions.hpp:232-239, float32 step by step
  query_rerank                       BitVecEngine.cpp:454-466, :521-535 (earlyAbandonRank = false)
"""
from __future__ import annotations

import numpy as np

import fast_ref

FLT_MAX = np.finfo(np.float32).max


def hamming_dists(rows: np.ndarray, queries: np.ndarray) -> np.ndarray:
    """rows uint64 [n][W], queries uint64 [nq][W] -> int64 [nq][n]."""
    rows = np.ascontiguousarray(rows, np.uint64)
    queries = np.ascontiguousarray(queries, np.uint64)
    out = np.zeros((queries.shape[0], rows.shape[0]), np.int64)
    rb = rows.view(np.uint8).reshape(rows.shape[0], -1)
    for q in range(queries.shape[0]):
        x = rb ^ queries[q:q + 1].view(np.uint8).reshape(1, -1)
        out[q] = np.unpackbits(x, axis=1).sum(axis=1, dtype=np.int64)
    return out


def query_sort(rows, queries, k: int, id_base: int = 0):
    """BitVecEngine::query(queries, k, Sort): (labels int32 [nq][k], dist uint32 [nq][k]); slots past min(k, n) are
    -1 / 0xffffffff."""
    d = hamming_dists(rows, queries)
    nq = d.shape[0]
    lab = np.full((nq, k), -1, np.int32)
    dis = np.full((nq, k), 0xffffffff, np.uint32)
    for q in range(nq):
        l, _ = fast_ref.knn_from_dists(d[q], k)
        ok = l >= 0
        lab[q, ok] = l[ok] + id_base
        dis[q, ok] = d[q][l[ok]]
    return lab, dis


def std_sort_perm_f32(dists) -> np.ndarray:
    """fast_ref.std_sort_perm over float32 distances (that one truncates to int): the same introsort helpers, which
    compare item[1] with <."""
    f = [(i, np.float32(d)) for i, d in enumerate(dists)]
    n = len(f)
    if n > 1:
        fast_ref._introsort_loop(f, 0, n, 2 * (n.bit_length() - 1))
        if n > 16:
            fast_ref._insertion_sort(f, 0, 16)
            for i in range(16, n):
                fast_ref._linear_insert(f, i)
        else:
            fast_ref._insertion_sort(f, 0, n)
    return np.array([p[0] for p in f], np.int64)


def knn_from_dists_indices_supplied(dists, indices, k: int):
    """KNNFromDistsIndicesSupplied as written: std::sort of the first k pairs, maybeInsertNeighbor
    (utils/Experiment.hpp:22-37) for the others.  len(dists) >= k.  Returns (idx int32 [k], dist float32 [k])."""
    d = np.asarray(dists, np.float32)
    idx = np.asarray(indices, np.int64)
    assert d.shape[0] >= k > 0
    head = std_sort_perm_f32(d[:k])
    ret = [(int(idx[p]), d[p]) for p in head]
    for i in range(k, d.shape[0]):
        if d[i] < ret[-1][1]:
            ret[-1] = (int(idx[i]), d[i])
            j = k - 1
            while j > 0 and ret[j - 1][1] > d[i]:
                ret[j - 1], ret[j] = ret[j], ret[j - 1]
                j -= 1
    return np.array([r[0] for r in ret], np.int32), np.array([r[1] for r in ret], np.float32)


def euclidean_no_sqrt(q: np.ndarray, X: np.ndarray) -> np.ndarray:
    """distance += (q[i] - x[i]) * (q[i] - x[i]) from 0.0f in dimension order, every step rounded to float32, for
    every row of X at once."""
    q = np.asarray(q, np.float32)
    X = np.asarray(X, np.float32)
    acc = np.zeros(X.shape[0], np.float32)
    for i in range(q.shape[0]):
        t = (q[i] - X[:, i]).astype(np.float32)
        acc = (acc + (t * t).astype(np.float32)).astype(np.float32)
    return acc


def query_rerank(rows, queries, X, XQ, k: int, factor: int, id_base: int = 0):
    """BitVecEngine::queryRerank(queries, oriQueries, k, factor, Sort, false): (labels int32 [nq][k], squared
    distances float32 [nq][k]); slots past min(k, kTemp) are -1 / FLT_MAX."""
    n = np.asarray(rows).shape[0]
    k_temp = min(factor * k, n)
    nq = np.asarray(queries).shape[0]
    lab = np.full((nq, k), -1, np.int32)
    dis = np.full((nq, k), FLT_MAX, np.float32)
    if k_temp == 0:
        return lab, dis
    cand, _ = query_sort(rows, queries, k_temp)
    kk = min(k, k_temp)
    for q in range(nq):
        d = euclidean_no_sqrt(XQ[q], np.asarray(X)[cand[q]])
        i, dd = knn_from_dists_indices_supplied(d, cand[q], kk)
        lab[q, :kk] = i + id_base
        dis[q, :kk] = dd
    return lab, dis
