"""KMeans::fit (KMeans.hpp:42-107) with given seeds, restated in float32.  The loops are the reference's; only what is
independent runs as one array operation: a sum over the dimensions is carried for all (row, centre) pairs at once, one
dimension after the other, and a centre's sum for all dimensions at once, one row after the other."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def fit(X, seed_rows, max_iter=25, root=True):
    """(centres [T][D], belongs_to [n], iterations); root=False compares the sums themselves (what the fit must NOT do)."""
    X = np.asarray(X).astype(np.float32)
    n, D = X.shape
    means = X[np.asarray(seed_rows)].copy()
    T, it = len(means), 0
    changed = True
    with np.errstate(all="ignore"):
        while changed and it < max_iter:
            dist = np.zeros((n, T), np.float32)
            for d in range(D):  # euclideanDistNoSQRT: distance += (a - b) * (a - b), every step rounded
                t = X[:, d, None] - means[None, :, d]
                dist += t * t
            if root:
                dist = np.sqrt(dist)
            dist_min, belongs = np.full(n, FLT_MAX), np.full(n, -1, np.int32)
            for j in range(T):  # the first centre with dist < dist_min
                take = dist[:, j] < dist_min
                dist_min[take], belongs[take] = dist[take, j], j
            assert (belongs >= 0).all(), "a row without a centre: the reference indexes new_centroids[-1]"
            new, count = np.zeros((T, D), np.float32), np.zeros(T, np.int32)
            for i in range(n):  # in row order, one accumulator per (centre, dimension)
                new[belongs[i]] += X[i]
                count[belongs[i]] += 1
            new /= count.astype(np.float32)[:, None]
            changed = False
            for c in range(T):
                if not (new[c] == means[c]).all():  # std::vector's ==
                    changed, means[c] = True, new[c]
            it += 1
    return means, belongs, it


def root_case():
    """Row 2 against centre 0: 1 + fl(t * t) = 1 + 2^-23 (t = 2^-11.5 rounded), against centre 1: 1.0.  Both roots are
    1.0f, so centre 0 wins; by the sums centre 1 would.  D = 2: at D = 1 a sum is one square and sqrtf gives |t| back."""
    X = np.array([[1.0, 2.0 ** -11.5], [1.0, 0.0], [0.0, 0.0]], np.float32)
    return X, [0, 1]
