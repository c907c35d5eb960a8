"""computeClusterIndex (utils/Experiment.hpp:372-392) restated in float32 NumPy: the checker of the cluster index."""
import numpy as np

import bitvec_ref as br

FLT_MAX = np.finfo(np.float32).max


def cluster_index(X, centroids):
    """(idx int32 [n], dist float32 [n]): for the centres in order, one float32 accumulator in dimension order, taken
    where dist < nearestDist from (-1, FLT_MAX).  (x - c) * (x - c) and (c - x) * (c - x) are the same float."""
    X = np.asarray(X, np.float32)
    idx = np.full(X.shape[0], -1, np.int32)
    best = np.full(X.shape[0], FLT_MAX, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c, centre in enumerate(np.asarray(centroids, np.float32)):
            d = br.euclidean_no_sqrt(centre, X)
            take = d < best
            best[take] = d[take]
            idx[take] = c
    return idx, best
