"""Plain restatement of the triangle-inequality form's answer, the checker of tests/test_bitvec_ti_gpu.py: the k smallest
of ALL rows by (sqrtf(euclideanDistNoSQRT), row).  No centre appears: the answer does not depend on them."""
import numpy as np

import bitvec_ref as br


def dists(q, X) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.sqrt(br.euclidean_no_sqrt(q, X)).astype(np.float32)


def query_naive_ti(X, XQ, k: int, id_base: int = 0):
    """(labels int32 [nq][k], distances float32 [nq][k]); slots past min(k, n) are -1 / FLT_MAX."""
    X = np.asarray(X, np.float32)
    nq, n = len(XQ), len(X)
    lab = np.full((nq, k), -1, np.int32)
    dis = np.full((nq, k), br.FLT_MAX, np.float32)
    for q in range(nq):
        d = dists(XQ[q], X)
        best = np.lexsort((np.arange(n), d))[:k]
        lab[q, :len(best)] = best + id_base
        dis[q, :len(best)] = d[best]
    return lab, dis
