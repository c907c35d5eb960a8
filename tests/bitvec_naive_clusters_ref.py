"""Plain restatement of BitVecEngine::queryNaiveWithClusterInfo with QueryMethod::Sort (BitVecEngine.cpp:875-918), the
checker of tests/test_bitvec_naive_clusters_gpu.py: the cluster form's candidates (bitvec_clusters_ref), every one's
euclideanDistNoSQRT and KNNFromDistsIndicesSupplied over them (bitvec_ref)."""
import numpy as np

import bitvec_clusters_ref as cr
import bitvec_ref as br


def query_naive_clusters(X, centroids, clust_idx, XQ, k: int, atleast: int = 1, id_base: int = 0):
    """(labels int32 [nq][k], squared distances float32 [nq][k]); slots past the candidates are -1 / FLT_MAX."""
    nq = len(XQ)
    lab = np.full((nq, k), -1, np.int32)
    dis = np.full((nq, k), br.FLT_MAX, np.float32)
    for q in range(nq):
        cand = cr.candidates(centroids, clust_idx, XQ[q], k, atleast)
        kk = min(k, len(cand))
        if kk:
            with np.errstate(over="ignore"):
                d = br.euclidean_no_sqrt(XQ[q], np.asarray(X)[cand])
            i, dd = br.knn_from_dists_indices_supplied(d, cand, kk)
            lab[q, :kk] = i + id_base
            dis[q, :kk] = dd
    return lab, dis
