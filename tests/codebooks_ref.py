"""NumPy restatement of the subspace codebook fit -- KMeans::staticFitSampling (KMeans.hpp:487-616) as VAQ.cpp:644-649
calls it, once per subspace on XTrain.block(0, s * L, n, L), each call sampling for itself -- and the inputs of the fixtures under
tests/golden/codebooks/ (regenerated here from a seed; the fixtures hold the reference's outputs and a digest of
these inputs).  The Lloyd loop, the permutation and the comparison are tests/kmeans_ref.py's, untouched.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

from kmeans_ref import assert_centres_equal, assign, fit, permutation_head  # noqa: F401  (re-exported to the tests)
import primitives_ref as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codebooks")
MAX_ITER = 25            # VAQ.cpp:648
ROWS_PER_CENTRE = 256    # KMeans.hpp:489
MIN_SAMPLE = 256 * 256   # KMeans.hpp:489
NOISE = 0.25             # a blob of make_inputs is a 5-level lattice of this step (settles fast); the centres spread 6

# name: (n, D, M, bits, kind, salt).  kind: "float" gaussian blobs, "bytes" uint8 rows with values 0..3, "bits01"
# uint8 rows with values 0..1, "rotated" float rows with a random orthogonal eigvec in front.  salt: part of the seed (ISSUE: a recorded run must show what
# its row of the table names)
CASES = {
    "tiny": (300, 8, 4, (1, 2, 3, 4), "float", 3),
    "odd": (4001, 24, 2, (5, 3), "float", 0),
    "sampled": (70000, 16, 2, (8, 5), "float", 0),
    "prefix": (140000, 8, 2, (9, 3), "float", 0),
    "bytes": (5000, 8, 4, (5, 5, 2, 2), "bytes", 0),
    "wide": (301, 512, 1, (3,), "float", 0),
    "rotated": (3000, 16, 4, (4, 4, 4, 4), "rotated", 2),
    # sampling decided per subspace: the 512-centre subspace takes all rows in order, its neighbours sample 65536
    "mixed": (66000, 6, 3, (3, 9, 5), "float", 0),
    # launch shapes of the assign kernel (tests/golden/codebooks/README.md): centres staged in more than one turn ...
    "staged": (5000, 24, 2, (9, 3), "float", 0),
    "dupes": (20000, 8, 1, (10,), "bits01", 0),
    # ... both sides of every boundary between its row tiles (L = D / 2) ...
    "tier40": (321, 80, 2, (3, 2), "float", 0),
    "tier41": (321, 82, 2, (3, 2), "float", 0),
    "tier80": (321, 160, 2, (3, 2), "float", 0),
    "tier81": (321, 162, 2, (3, 2), "float", 1),
    "tier160": (321, 320, 2, (3, 2), "float", 2),
    "tier161": (321, 322, 2, (3, 2), "float", 0),
    # ... the global-memory path in more than one turn, and two odd slice lengths
    "wide_staged": (333, 161, 1, (5,), "float", 0),
    "len1": (600, 2, 2, (2, 3), "float", 1),
    "len27": (600, 54, 2, (2, 3), "float", 0),
}
TIERS = {"tier40": 40, "tier41": 41, "tier80": 80, "tier81": 81, "tier160": 160, "tier161": 161}
STAGE_FLOATS = 4096      # floats of centres the assign kernel stages in LDS at a time (vaq_codebooks.hip)
TILE_BYTES = 40 * 1024   # LDS its tile of slices may take


def assign_launch(L: int, k_max: int):
    """(rows per workgroup, tile in LDS?, centres per stage) of cb_assign_kernel, from the rules of codebooks_fit."""
    R = 256
    while R > 64 and R * L * 4 > TILE_BYTES:
        R >>= 1
    return R, R * L * 4 <= TILE_BYTES, max(1, min(k_max, STAGE_FLOATS // L))


def make_inputs(name: str):
    """(X n x D float32 or uint8, eigvec D x D float32 or None) of a case, from its fixed seed."""
    n, D, M, bits, kind, salt = CASES[name]
    rng = np.random.default_rng(int(hashlib.sha256(("codebooks:%s:%d" % (name, salt)).encode()).hexdigest()[:8], 16))
    if kind == "bytes":
        return rng.integers(0, 4, size=(n, D), dtype=np.int64).astype(np.uint8), None
    if kind == "bits01":
        return rng.integers(0, 2, size=(n, D), dtype=np.int64).astype(np.uint8), None
    L = D // M
    X = np.empty((n, D), np.float32)
    for s in range(M):  # per subspace: as many gaussian blobs as centres, so that some subspaces settle early
        blobs = (rng.normal(size=(1 << bits[s], L)) * 6).astype(np.float32)
        X[:, s * L:(s + 1) * L] = blobs[rng.integers(0, len(blobs), n)] + (rng.integers(-2, 3, size=(n, L)) * NOISE).astype(np.float32)
    if kind != "rotated":
        return X, None
    q, _ = np.linalg.qr(rng.normal(size=(D, D)))  # the blobs are those of the projected rows
    eig = np.ascontiguousarray(q, np.float32)
    return np.ascontiguousarray(X @ eig.T, np.float32), eig


def digest(X, eig) -> str:
    h = hashlib.sha256()
    for a in [X] + ([eig] if eig is not None else []):
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def load_fixture(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def sample_count(n: int, k: int) -> int:
    """Rows staticFitSampling works on for k centres out of n rows."""
    return min(n, max(ROWS_PER_CENTRE * k, MIN_SAMPLE))


def sampled(n: int, k: int) -> bool:
    """KMeans.hpp:493, decided by every call for itself: more rows than its sample size."""
    return n > sample_count(n, k)


def projected_rows(X, eig):
    """All rows, widened and projected."""
    P = np.ascontiguousarray(X, np.float32)
    return pr.project32(P, eig) if eig is not None else P


def projected_sample(X, eig, bits):
    """The rows the largest SAMPLED subspace works on, in the reference's order, widened and projected (only these
    rows: a row's projection does not depend on the others); every sampled subspace works on a prefix of it.  No
    subspace samples: all rows in their own order."""
    n = X.shape[0]
    S = max([sample_count(n, 1 << b) for b in bits if sampled(n, 1 << b)], default=0)
    return projected_rows(X[permutation_head(n, S)] if S else X, eig)


def subspace_rows(P, n, D, M, bits, s, full=None):
    """What the reference's call for subspace s sees after its own sampling: dense rows of L floats.  P: the
    projected sample; full: all rows projected, read by a subspace that does not sample (None: no subspace samples
    and P holds them)."""
    L = D // M
    k = 1 << bits[s]
    src = P[:sample_count(n, k)] if sampled(n, k) or full is None else full
    assert len(src) == sample_count(n, k)
    return np.ascontiguousarray(src[:, s * L:(s + 1) * L])


def fit_codebooks(X, M, bits, eig=None, max_iter: int = MAX_ITER):
    """([M centre matrices k_s x L], [iterations], [NaN-row masks])"""
    n, D = X.shape
    P = projected_sample(X, eig, bits)
    mixed = len({sampled(n, 1 << b) for b in bits}) == 2
    full = projected_rows(X, eig) if mixed else None
    cents, iters, nans = [], [], []
    for s in range(M):
        means, it = fit(subspace_rows(P, n, D, M, bits, s, full), 1 << bits[s], max_iter)
        cents.append(means)
        iters.append(it)
        nans.append(np.isnan(means).any(axis=1))
    return cents, iters, nans
