"""BitVecEngine's two encoders restated in plain NumPy loops over projected values: the sign form (BitVecEngine.hpp:239-255)
and the quantile form (:509-590: the quantile expression, the first-match scan over the raw thresholds, a bit-stream
writer), and the cases the CPU and GPU tests share.  No compiled reference: the header needs glpk.h."""
import functools
import math

import numpy as np

import lutfit_ref as lr

F = np.float32
FLT_MAX = np.finfo(F).max
U = np.uint64


def set_bit(out, i, p):
    out[i, p // 64] |= U(1) << U(63 - p % 64)


def sign_ref(Xp):
    n, D = Xp.shape
    out = np.zeros((n, (D + 63) // 64), U)
    for i in range(n):
        for d in range(D):
            if Xp[i, d] > 0:
                set_bit(out, i, d)
    return out


def thresholds_ref(Xp, bits, fill=0.0):
    """[D][256]: T[q] = quantile(Z, 2^b - 1)[q], then FLT_MAX; entries nothing writes hold `fill`"""
    n, D = Xp.shape
    T = np.full((D, 256), fill, F)
    for d, b in enumerate(bits):
        if b == 0:
            continue
        Z = lr.sort_column(Xp[:, d])
        for i in range((1 << b) - 1):
            poi = lr.quantile_pos(i, 1 << b, n)  # p = (float)(i + 1) / (N + 1), N + 1 = 2^b
            left, right = max(int(math.floor(poi)), 0), min(int(math.ceil(poi)), n - 1)
            f = F(poi - F(left))
            T[d, i] = F(F(F(1) - f) * Z[left]) + F(f * Z[right])
        T[d, (1 << b) - 1] = FLT_MAX
    return T


def quantile_ref(Xp, bits, T):
    n = Xp.shape[0]
    out = np.zeros((n, (sum(bits) + 63) // 64), U)
    pos = 0
    for j, b in enumerate(bits):
        for i in range(n if b else 0):
            with np.errstate(invalid="ignore"):
                hits = np.nonzero(Xp[i, j] <= T[j, :1 << b])[0]  # the first q with x <= Q(q, j); none: nothing is ORed
            for k in range(b if hits.size else 0):
                if (int(hits[0]) >> (b - 1 - k)) & 1:
                    set_bit(out, i, pos + k)
        pos += b
    return out


def tile_rows(D):
    """bitvec_encode_tile_rows: 4 waves x 16 rows, halved while the tile passes 32 KB"""
    r = 16
    while r > 1 and 4 * r * ((D + 3) & ~3) > 8192:
        r >>= 1
    return 4 * r


SIGN_DIMS = (1, 64, 65, 100, 128, 192, 1024)
SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 2.5], F)  # rows 0..7 of column 0 and D - 1

# nine 7-bit codes then a 3-bit one over bits 63..65, 0-bit dimensions, 1 and 8 bits, 75 bits; a code that ends at
# bit 64, 69 bits; 1024 bits, whose 32768 thresholds do not fit the workgroup's LDS
ALLOCS = {"straddle": [7] * 9 + [3, 0, 1, 0, 8], "ends64": [8] * 7 + [4, 4, 0, 5], "full1024": [8] * 128}


@functools.lru_cache(maxsize=None)
def quantile_case(name):
    """(bits, training rows, their thresholds, rows to encode): column 0 is constant (thresholds an ulp apart, not
    monotone); two tiles + 1 training rows, rows 1..5 replaced by a threshold of each column, a value above the training
    range (<= FLT_MAX: the last code), +inf and NaN (no q matches: nothing is ORed) and -inf (code 0)."""
    bits = ALLOCS[name]
    D = len(bits)
    rs = np.random.RandomState(len(name))
    train = (rs.standard_normal((300, D)) * 9).astype(F)
    train[:, 0] = F(3.7)
    T = thresholds_ref(train, bits)
    rows = train[np.arange(2 * tile_rows(D) + 1) % 300].copy()
    rows[1] = [T[d, (1 << b) // 2 - 1] if b else 0 for d, b in enumerate(bits)]
    rows[2:6] = np.array([train.max() + 1, np.inf, np.nan, -np.inf], F)[:, None]
    return bits, train, T, rows
