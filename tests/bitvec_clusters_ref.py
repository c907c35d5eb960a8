"""Plain restatement of BitVecEngine::queryWithClusterInfo / ::queryRerankWithClusterInfo with QueryMethod::Sort
(BitVecEngine.cpp:259-304, :553-568), the checker of tests/test_bitvec_clusters_*.py, composed from tests/bitvec_ref.py.
Where the candidates number fewer than k (the reference reads past its arrays) the slots behind them are empty."""
from __future__ import annotations

import numpy as np

import bitvec_ref as br


def candidates(centroids, clust_idx, oq, k: int, atleast: int) -> np.ndarray:
    """The rows one query visits, in visiting order: the centres by std::sort under distance alone, walked until their
    members number k and the centres atleast; a cluster's members in ascending row order."""
    clust_idx = np.asarray(clust_idx)
    T = len(centroids)
    assert 1 <= atleast <= T
    members = [np.flatnonzero(clust_idx == c) for c in range(T)]
    order = br.std_sort_perm_f32(br.euclidean_no_sqrt(oq, centroids))
    visit = cum = 0
    for c in order:
        visit += 1
        cum += len(members[c])
        if cum >= k:
            break
    visit = max(visit, atleast)
    return np.concatenate([members[c] for c in order[:visit]]).astype(np.int64)


def query_clusters(rows, queries, centroids, clust_idx, ori_queries, k: int, atleast: int = 1, id_base: int = 0):
    """(labels int32 [nq][k], dist uint32 [nq][k]); empty slots -1 / 0xffffffff."""
    nq = np.asarray(queries).shape[0]
    lab = np.full((nq, k), -1, np.int32)
    dis = np.full((nq, k), 0xffffffff, np.uint32)
    for q in range(nq):
        cand = candidates(centroids, clust_idx, ori_queries[q], k, atleast)
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
