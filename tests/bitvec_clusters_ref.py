"""Plain restatement of BitVecEngine::queryWithClusterInfo / ::queryRerankWithClusterInfo with QueryMethod::Sort
(BitVecEngine.cpp:259-304, :553-568), the checker of tests/test_bitvec_clusters_*.py, composed from tests/bitvec_ref.py.
Where the candidates number fewer than k (the reference reads past its arrays) the slots behind them are empty.

A centre distance that is NaN (a NaN coordinate in a query or a centre) puts std::sort outside what C++ defines: the
comparator is no strict weak order then.  The answer pinned here is the restated sort's (bitvec_ref.std_sort_perm_f32:
every comparison with a NaN is false, every scan stops at the first false comparison), which tests/cpp/
cluster_sort_test.cpp holds against vaq::stdsort::sort_by<12, true> under ClusterLt on the same arrays.

`dist` is the arithmetic of the centre distances: the reference's by default; tests/bitvec_clusters_cases.py passes a
fused one to show that an input tells the two apart."""
from __future__ import annotations

import numpy as np

import bitvec_ref as br


def centre_order(centroids, oq, dist=br.euclidean_no_sqrt) -> np.ndarray:
    """The centres in visiting order: std::sort of the (c, dist) pairs under distance alone."""
    with np.errstate(over="ignore", invalid="ignore"):
        return br.std_sort_perm_f32(dist(oq, centroids))


def visited(centroids, clust_idx, oq, k: int, atleast: int, dist=br.euclidean_no_sqrt) -> np.ndarray:
    """The clusters one query walks, in visiting order (the empty ones too): the centres by std::sort under distance
    alone, walked until their members number k and the centres atleast."""
    T = len(centroids)
    assert 1 <= atleast <= T
    sizes = np.bincount(np.asarray(clust_idx, np.int64), minlength=T)
    order = centre_order(centroids, oq, dist)
    visit = cum = 0
    for c in order:
        visit += 1
        cum += sizes[c]
        if cum >= k:
            break
    return order[:max(visit, atleast)]


def candidates(centroids, clust_idx, oq, k: int, atleast: int, dist=br.euclidean_no_sqrt) -> np.ndarray:
    """The rows one query visits, in visiting order: cluster after cluster of visited(), a cluster's members in
    ascending row order."""
    clust_idx = np.asarray(clust_idx)
    walk = visited(centroids, clust_idx, oq, k, atleast, dist)
    return np.concatenate([np.flatnonzero(clust_idx == c) for c in walk]).astype(np.int64)


def query_clusters(rows, queries, centroids, clust_idx, ori_queries, k: int, atleast: int = 1, id_base: int = 0,
                   dist=br.euclidean_no_sqrt):
    """(labels int32 [nq][k], dist uint32 [nq][k]); empty slots -1 / 0xffffffff."""
    nq = np.asarray(queries).shape[0]
    lab = np.full((nq, k), -1, np.int32)
    dis = np.full((nq, k), 0xffffffff, np.uint32)
    for q in range(nq):
        cand = candidates(centroids, clust_idx, ori_queries[q], k, atleast, dist)
        kk = min(k, len(cand))
        if kk == 0:
            continue
        d = br.hamming_dists(np.asarray(rows)[cand], np.asarray(queries)[q:q + 1])[0]
        i, dd = br.knn_from_dists_indices_supplied(d, cand, kk)
        lab[q, :kk] = i + id_base
        dis[q, :kk] = dd.astype(np.uint32)
    return lab, dis


def query_rerank_clusters(rows, queries, centroids, clust_idx, X, XQ, k: int, factor: int, atleast: int = 1, id_base: int = 0):
    """(labels int32 [nq][k], squared distances float32 [nq][k]); slots past min(k, kTemp) are -1 / FLT_MAX."""
    n, nq = np.asarray(rows).shape[0], np.asarray(queries).shape[0]
    k_temp = min(factor * k, n)
    lab = np.full((nq, k), -1, np.int32)
    dis = np.full((nq, k), br.FLT_MAX, np.float32)
    if k_temp == 0:
        return lab, dis
    cand, _ = query_clusters(rows, queries, centroids, clust_idx, XQ, k_temp, atleast)
    kk = min(k, k_temp)
    for q in range(nq):
        d = br.euclidean_no_sqrt(XQ[q], np.asarray(X)[cand[q]])
        i, dd = br.knn_from_dists_indices_supplied(d, cand[q], kk)
        lab[q, :kk] = i + id_base
        dis[q, :kk] = dd
    return lab, dis
