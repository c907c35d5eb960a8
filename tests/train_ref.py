"""Shared by tests/test_train_cpu.py and tests/test_train_gpu.py: the inputs of the fixtures under tests/golden/train
(regenerated from a seed, guarded by a digest), and plain numpy restatements of what the library documents for the
training front half -- the rows and summation order of the second moment, the Jacobi solver of vaq_train_rot.h, the
brute-force ILP -- plus thin ctypes wrappers of the host entry points."""
from __future__ import annotations

import ctypes as C
import hashlib
import itertools
import os
import zlib

import numpy as np

from kmeans_ref import permutation_head  # noqa: F401  (randomPermutation's head, mt19937(13517106))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train")
TILE = 1024
MAX_SWEEPS = 60

# name: (n, D, M, percent_var, min_bits, max_bits, bit_budget)
CASES = {
    "tiny": (300, 8, 4, 1.0, 1, 8, 16),
    "balance_kept": (2000, 16, 4, 1.0, 1, 8, 16),
    "balance_undone": (2000, 16, 4, 1.0, 1, 8, 16),
    "percent": (2000, 16, 4, 0.9, 1, 8, 8),
    "percent_two": (2000, 16, 4, 0.9, 1, 8, 12),
    "sampled": (2001, 2, 2, 1.0, 1, 8, 8),
    "bytes": (4000, 16, 4, 1.0, 1, 8, 16),
    "deficient": (6, 8, 4, 1.0, 1, 8, 16),
}
# the spectra XtX is given (n > D cases; the rows are an orthonormal basis scaled by their roots and turned)
SPECTRA = {
    "tiny": [90.0, 40.0, 22.0, 12.0, 7.0, 4.0, 2.5, 1.2],
    "balance_kept": [100.0, 9.0, 8.0, 7.0, 6.0, 5.5, 5.0, 4.5, 4.0, 3.6, 3.2, 2.9, 2.5, 2.2, 2.0, 1.8],
    "balance_undone": [10.0, 9.8, 2.4, 2.2, 2.0, 1.9, 1.8, 0.3, 0.27, 0.24, 0.21, 0.18, 0.15, 0.12, 0.1, 0.06],
    "percent": [3000.0, 20.0, 15.0, 10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.5, 4.0, 3.5, 3.0, 2.5, 2.0, 1.5],
    "percent_two": [300.0, 100.0, 60.0, 40.0, 110.0, 90.0, 70.0, 52.0, 31.0, 26.0, 22.0, 18.0, 33.0, 21.0, 15.0, 12.0],
    "sampled": [50.0, 7.0],
}


def _seed(name: str) -> int:
    return zlib.crc32(("train/" + name).encode())


def make_inputs(name: str) -> np.ndarray:
    """The rows of a case: float32, or uint8 for `bytes`."""
    n, D = CASES[name][:2]
    rng = np.random.Generator(np.random.PCG64(_seed(name)))
    if name == "bytes":
        turn, _ = np.linalg.qr(rng.standard_normal((D, D)))
        Z = rng.standard_normal((n, D)) * (40.0 * 0.8 ** np.arange(D))
        return np.clip(np.rint(128.0 + Z @ turn.T), 0, 255).astype(np.uint8)
    if name == "deficient":
        return rng.standard_normal((n, D)).astype(np.float32)
    spec = np.array(sorted(SPECTRA[name], reverse=True))
    Q, _ = np.linalg.qr(rng.standard_normal((n, D)))
    turn, _ = np.linalg.qr(rng.standard_normal((D, D)))
    return ((Q * np.sqrt(spec)) @ turn.T).astype(np.float32)


def digest(X: np.ndarray) -> str:
    return hashlib.sha256(str(X.dtype).encode() + str(X.shape).encode() + np.ascontiguousarray(X).tobytes()).hexdigest()


def load_fixture(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ---- the second moment ----
def sample_rows(n: int, D: int):
    """The rows the moment sums, in the order it sums them (VAQ.cpp:17-24)."""
    s = 1000 * D
    return np.asarray(permutation_head(n, s), np.int64) if s < n else np.arange(n, dtype=np.int64)


def moment_ref(X: np.ndarray) -> np.ndarray:
    """The documented order: tiles of 1024 sample positions; within a tile the (exact) products added in ascending
    position from +0; the tile partials added in ascending tile order from +0.  All in double."""
    n, D = X.shape
    S = X[sample_rows(n, D)].astype(np.float64)
    total = np.zeros((D, D))
    for t0 in range(0, S.shape[0], TILE):
        part = np.zeros((D, D))
        for x in S[t0:t0 + TILE]:
            part = part + np.multiply.outer(x, x)
        total = total + part
    return total


def moment_abs(X: np.ndarray) -> np.ndarray:
    """sum_r |x_ri x_rj| over the rows summed: what the gamma_n bound scales."""
    n, D = X.shape
    S = np.abs(X[sample_rows(n, D)].astype(np.float64))
    return S.T @ S


def gamma(n: int) -> float:
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


# ---- the Jacobi solver (vaq_train_rot.h restated) ----
def jacobi_pairs(D: int, r: int):
    n = D + (D & 1)
    m = n - 1
    out = []
    for i in range(n // 2):
        a, b = (m, r % m) if i == 0 else ((r + i) % m, (r - i + m) % m)
        if a < D and b < D:
            out.append((min(a, b), max(a, b)))
    return out


def jacobi_rot(app, aqq, apq):
    prod = abs(app * aqq)
    rotate = (apq != 0.0) if prod == 0.0 else abs(apq) > 2.0 ** -52 * np.sqrt(prod)
    if not rotate:
        return None
    with np.errstate(over="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    return c, t * c


def jacobi_finish(A0, V):
    """Every vector divided by its norm, its eigenvalue its Rayleigh quotient on A0; every sum in ascending index from
    +0, as vaq_train_rot.h adds them."""
    D = A0.shape[0]
    nrm = np.zeros(D)
    for i in range(D):
        nrm = nrm + V[i, :] * V[i, :]
    nrm = np.where(nrm > 0.0, np.sqrt(nrm), 1.0)
    Vn = V / nrm
    W = np.zeros((D, D))
    for k in range(D):
        W = W + np.multiply.outer(A0[:, k], Vn[k, :])
    lam = np.zeros(D)
    for i in range(D):
        lam = lam + Vn[i, :] * W[i, :]
    order = sorted(range(D), key=lambda i: -lam[i])  # (stable: equal values by ascending column)
    vec = Vn[:, order].copy()
    for j in range(D):
        big = int(np.argmax(np.abs(vec[:, j])))  # (the first of equal magnitudes)
        if vec[big, j] < 0.0:
            vec[:, j] = -vec[:, j]
    return np.array([lam[i] for i in order]), vec


def jacobi_ref(A: np.ndarray):
    """(values, vectors, sweeps) by the same steps as vaqhip_sym_eigen_host, element for element."""
    A = np.array(A, np.float64)
    A0 = A.copy()
    D = A.shape[0]
    V = np.eye(D)
    steps = 0 if D < 2 else D + (D & 1) - 1
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        rotated = 0
        for r in range(steps):
            pairs = jacobi_pairs(D, r)
            rots = [jacobi_rot(np.float64(A[p, p]), np.float64(A[q, q]), np.float64(A[p, q])) for p, q in pairs]
            for (p, q), rot in zip(pairs, rots):
                if rot is None:
                    continue
                rotated += 1
                c, s = rot
                for Mx in (A, V):
                    x, y = Mx[:, p].copy(), Mx[:, q].copy()
                    Mx[:, p] = c * x - s * y
                    Mx[:, q] = s * x + c * y
            for (p, q), rot in zip(pairs, rots):
                if rot is None:
                    continue
                c, s = rot
                x, y = A[p, :].copy(), A[q, :].copy()
                A[p, :] = c * x - s * y
                A[q, :] = s * x + c * y
                A[p, q] = 0.0
                A[q, p] = 0.0
        if not rotated:
            break
        sweeps += 1
    values, vectors = jacobi_finish(A0, V)
    return values, vectors, sweeps


def eigen_matrices():
    """name -> symmetric double matrix: the cases of the issue (the GPU file adds D = 129)."""
    rng = np.random.Generator(np.random.PCG64(_seed("eigen")))

    def sym(D):
        B = rng.standard_normal((D, D))
        return (B + B.T) / 2

    out = {"d1": np.array([[3.5]]), "d2": sym(2), "d3": sym(3), "d5": sym(5), "d64": sym(64),
           "diagonal": np.diag([4.0, -1.0, 9.0, 0.5, 9.0, 2.0]), "zero": np.zeros((7, 7))}
    v = rng.standard_normal(12)
    out["repeated"] = 2.5 * np.eye(12) + np.multiply.outer(v, v)
    Q, _ = np.linalg.qr(rng.standard_normal((24, 24)))
    G = (Q * 10.0 ** np.linspace(6, -6, 24)) @ Q.T
    out["graded"] = (G + G.T) / 2
    return out


def eigh_quality(A, values, vectors):
    """(residual max|A v - lambda v|, orthogonality max|VtV - I|) of a decomposition."""
    res = np.max(np.abs(A @ vectors - vectors * values)) if A.size else 0.0
    orth = np.max(np.abs(vectors.T @ vectors - np.eye(A.shape[0])))
    return float(res), float(orth)


# ---- the ILP by enumeration ----
def brute_force_bits(c, lb, max_bits, k, budget):
    """(bits, objective) or None: every allocation, the objective summed in double in ascending i, the
    lexicographically greatest among those that reach the optimum."""
    H = len(c)
    cd = [float(np.float32(x)) for x in c]
    best, arg = None, None
    for x in itertools.product(*[range(lb[i], max_bits + 1) for i in range(H)]):
        if sum(x) != budget or any(x[i] - x[i + 1] > k[i] for i in range(H - 1)):
            continue
        obj = cd[0] * x[0]
        for i in range(1, H):
            obj = obj + cd[i] * x[i]
        if best is None or obj > best or (obj == best and x > arg):
            best, arg = obj, x
    return None if best is None else (list(arg), best)


# ---- the host entry points ----
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def train_plan(lib, eig, M, percent_var, min_bits, max_bits):
    eig = np.ascontiguousarray(eig, np.float32)
    D = eig.shape[0]
    srt, order = np.zeros(D, np.int32), np.zeros(D, np.int32)
    var, cum = np.zeros(max(M, 1), np.float32), np.zeros(max(M, 1), np.float32)
    lb, k = np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1), np.int32)
    hi, kept = C.c_int(0), C.c_int(0)
    rc = lib.vaqhip_train_plan(_p(eig), D, M, percent_var, min_bits, max_bits, _p(srt), _p(order), _p(var), _p(cum),
                               C.byref(hi), _p(lb), _p(k), C.byref(kept))
    if rc:
        return rc
    H = hi.value
    return dict(sorted=srt, order=order, var=var[:M], cum=cum[:M], highest=H, lb=lb[:H], k=k[:max(H - 1, 0)],
                swaps_kept=kept.value)


def allocate_bits(lib, c, lb, max_bits, k, budget):
    c = np.ascontiguousarray(c, np.float32)
    H = c.shape[0]
    lb = np.ascontiguousarray(lb, np.int32)
    k = np.ascontiguousarray(np.concatenate([np.asarray(k, np.int64), [0]]), np.int32)
    bits = np.zeros(H, np.int32)
    obj = C.c_double(0)
    rc = lib.vaqhip_allocate_bits(_p(c), H, _p(lb), max_bits, _p(k), budget, _p(bits), C.byref(obj))
    return rc if rc else (bits.tolist(), obj.value)


def sym_eigen_host(lib, A):
    A = np.array(A, np.float64, order="C")
    D = A.shape[0]
    values, vectors = np.zeros(D), np.zeros((D, D))
    sweeps = C.c_int(-1)
    rc = lib.vaqhip_sym_eigen_host(_p(A), D, _p(values), _p(vectors), C.byref(sweeps))
    return rc, values, vectors, sweeps.value
