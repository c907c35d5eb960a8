"""NumPy restatement of the reference's FAST search path (VAQ::searchFast,
VAQ.cpp:1778-1834) and of VAQ::learnQuantization (VAQ.cpp:1118-1187), the checker
of tests/test_fast_*.py.  tests/golden/fast/ pins it to the reference's own
functions (README.md there).

  small_quantize   utils/Math.hpp:215-224 (with the offsets of VAQ.cpp:1782-1789)
  row_dists        the ShuffleAVX2 + _mm256_adds_epi16 loop: never saturates here
  std_sort_perm    libstdc++ std::sort with a distance-only comparator
  knn_from_dists   utils/Experiment.hpp:22-56
  percentile       utils/Math.hpp:190-213
  random_permutation  utils/Random.hpp:18-28
  learn_quantization  VAQ.cpp:1118-1187 (loss summed in double)
"""
from __future__ import annotations

import numpy as np

ALPHAS = [np.float32(a) for a in (.001, .002, .005, .01, .02, .05, .1)]


def small_quantize(lut: np.ndarray, offsets: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """lut [..., M, ksub] float32 -> uint8: min(floor(max(lut - off, 0) * scale), 255),
    four float32 steps."""
    lut = np.asarray(lut, np.float32)
    off = np.asarray(offsets, np.float32)[:, None]
    sc = np.asarray(scale, np.float32)[:, None]
    x = np.maximum(lut - off, np.float32(0))
    x = (x * sc).astype(np.float32)
    return np.minimum(np.floor(x), np.float32(255)).astype(np.uint8)


def small_lut16(lut: np.ndarray, offsets, scale) -> np.ndarray:
    """vaqhip_build_small_lut's layout: [nq][M][16], entries >= ksub zero."""
    q = small_quantize(lut, offsets, scale)
    out = np.zeros(q.shape[:-1] + (16,), np.uint8)
    out[..., :q.shape[-1]] = q
    return out


def row_dists(small: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """small [M][>=ncent] uint8, codes [N][M] -> int64 [N]: sum_s small[s][code[s]]."""
    codes = np.asarray(codes, np.int64)
    M = codes.shape[1]
    return np.asarray(small, np.int64)[np.arange(M)[None, :], codes].sum(axis=1)


# ---------------------------------------------------------------------------- std::sort
def _lt(a, b):
    return a[1] < b[1]


def _adjust_heap(f, base, hole, length, value):
    top = hole
    second = hole
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if _lt(f[base + second], f[base + second - 1]):
            second -= 1
        f[base + hole] = f[base + second]
        hole = second
    if (length & 1) == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        f[base + hole] = f[base + second - 1]
        hole = second - 1
    parent = (hole - 1) // 2
    while hole > top and _lt(f[base + parent], value):
        f[base + hole] = f[base + parent]
        hole = parent
        parent = (hole - 1) // 2
    f[base + hole] = value


def _heap_sort(f, lo, hi):
    n = hi - lo
    if n >= 2:
        parent = (n - 2) // 2
        while True:
            _adjust_heap(f, lo, parent, n, f[lo + parent])
            if parent == 0:
                break
            parent -= 1
    last = n - 1
    while last > 0:
        v = f[lo + last]
        f[lo + last] = f[lo]
        _adjust_heap(f, lo, 0, last, v)
        last -= 1


def _median_to_first(f, r, a, b, c):
    def sw(i, j):
        f[i], f[j] = f[j], f[i]
    if _lt(f[a], f[b]):
        if _lt(f[b], f[c]):
            sw(r, b)
        elif _lt(f[a], f[c]):
            sw(r, c)
        else:
            sw(r, a)
    elif _lt(f[a], f[c]):
        sw(r, a)
    elif _lt(f[b], f[c]):
        sw(r, c)
    else:
        sw(r, b)


def _partition_pivot(f, lo, hi):
    mid = lo + (hi - lo) // 2
    _median_to_first(f, lo, lo + 1, mid, hi - 1)
    first, last = lo + 1, hi
    while True:
        while _lt(f[first], f[lo]):
            first += 1
        last -= 1
        while _lt(f[lo], f[last]):
            last -= 1
        if not first < last:
            return first
        f[first], f[last] = f[last], f[first]
        first += 1


def _introsort_loop(f, lo, hi, depth):
    while hi - lo > 16:
        if depth == 0:
            _heap_sort(f, lo, hi)
            return
        depth -= 1
        cut = _partition_pivot(f, lo, hi)
        _introsort_loop(f, cut, hi, depth)
        hi = cut


def _linear_insert(f, last):
    v = f[last]
    nxt = last - 1
    while _lt(v, f[nxt]):
        f[last] = f[nxt]
        last = nxt
        nxt -= 1
    f[last] = v


def _insertion_sort(f, lo, hi):
    if lo == hi:
        return
    for i in range(lo + 1, hi):
        if _lt(f[i], f[lo]):
            v = f[i]
            f[lo + 1:i + 1] = f[lo:i]
            f[lo] = v
        else:
            _linear_insert(f, i)


def std_sort_perm(dists) -> np.ndarray:
    """The order std::sort (libstdc++ introsort) leaves (idx, dist) pairs in under a
    distance-only comparator: returns the idx sequence."""
    f = [(i, int(d)) for i, d in enumerate(dists)]
    n = len(f)
    if n > 1:
        _introsort_loop(f, 0, n, 2 * (n.bit_length() - 1))
        if n > 16:
            _insertion_sort(f, 0, 16)
            for i in range(16, n):
                _linear_insert(f, i)
        else:
            _insertion_sort(f, 0, n)
    return np.array([p[0] for p in f], np.int64)


def knn_from_dists(dists, k: int):
    """KNNFromDists (utils/Experiment.hpp:40-56) as the k smallest by (dist, seq):
    seq = position in std::sort's output for rows < k, the row after.  N < k: the
    first N rows only, the rest -1 / FLT_MAX (the reference reads past its array).
    Returns (labels int64 [k], dists float32 [k])."""
    d = np.asarray(dists, np.int64)
    n = d.shape[0]
    kk = min(k, n)
    head = std_sort_perm(d[:kk])
    seq = np.arange(n, dtype=np.int64)
    seq[head] = np.arange(kk)
    order = np.lexsort((seq, d))[:kk]
    lab = np.full(k, -1, np.int64)
    dis = np.full(k, np.finfo(np.float32).max, np.float32)
    lab[:kk] = order
    dis[:kk] = d[order].astype(np.float32)
    return lab, dis


def search_fast(lut: np.ndarray, offsets, scale, codes: np.ndarray, k: int, id_base: int = 0):
    """Whole FAST search: lut [nq][M][ksub] (CreateLUT, zero-padded) -> labels, dists [nq][k]."""
    nq = lut.shape[0]
    labs = np.empty((nq, k), np.int64)
    dis = np.empty((nq, k), np.float32)
    for q in range(nq):
        sm = small_quantize(lut[q], offsets, scale)
        l, d = knn_from_dists(row_dists(sm, codes), k)
        labs[q] = np.where(l >= 0, l + id_base, -1)
        dis[q] = d
    return labs, dis


# --------------------------------------------------------------------------- learning
def percentile(col_sorted: np.ndarray, percent) -> np.float32:
    """utils/Math.hpp:190-213 on one ascending column, float32 as written."""
    percent = np.float32(percent)
    rows = col_sorted.shape[0]
    nthF = np.float32(percent * np.float32(rows - 1))
    fl = np.float32(np.floor(nthF))  # std::round (halves away from zero) of nthF >= 0
    r = np.float32(fl + np.float32(1)) if np.float32(nthF - fl) >= np.float32(0.5) else fl
    if abs(np.float32(r - nthF)) <= np.float32(0.00001):
        return np.float32(col_sorted[int(nthF)])
    f = np.float32(col_sorted[int(np.floor(nthF))])
    c = np.float32(col_sorted[int(np.ceil(nthF))])
    fraction = np.float32(nthF - r)
    return np.float32(f + np.float32(np.float32(c - f) * fraction))


def percentile_cols(x: np.ndarray, percent) -> np.ndarray:
    """percentile of every column of a (rows, cols) matrix."""
    return np.array([percentile(np.sort(x[:, j]), percent) for j in range(x.shape[1])], np.float32)


def random_permutation(n: int, seed: int = 13517106) -> np.ndarray:
    """utils/Random.hpp:18-28: std::mt19937(seed), i2 = i + mt() % (n - i)."""
    rs = np.random.RandomState(seed)  # init_genrand(seed): the std::mt19937(seed) state
    raw = rs._bit_generator.random_raw(max(n - 1, 0)) if n > 1 else np.empty(0, np.uint64)
    out = np.arange(n, dtype=np.int64)
    for i in range(n - 1):
        i2 = i + int(raw[i]) % (n - i)
        out[i], out[i2] = out[i2], out[i]
    return out


def learn_from_luts(luts: np.ndarray):
    """The alpha loop of VAQ::learnQuantization (VAQ.cpp:1160-1186) on the stacked tables
    luts (sample * ksub rows, M columns).  Returns (offsets, scale, alpha index)."""
    luts = np.asarray(luts, np.float32)
    best = float(np.finfo(np.float32).max)
    res = None
    for ai, a in enumerate(ALPHAS):
        floors = percentile_cols(luts, a)
        off = np.maximum(luts - floors[None, :], np.float32(0))
        ceil = percentile_cols(off, np.float32(np.float32(1) - a))
        sc = (np.float32(255) / ceil).astype(np.float32)
        q = np.minimum(np.floor((off * sc[None, :]).astype(np.float32)), np.float32(255)).astype(np.uint8)
        ideal = ((luts - off) * sc[None, :]).astype(np.float32) - q.astype(np.float32)
        loss = float(np.sum((ideal * ideal).astype(np.float32), dtype=np.float64))
        if loss <= best:
            best = loss
            res = (floors, sc, ai)
    return res


def stack_luts(lut_sample: np.ndarray) -> np.ndarray:
    """[sample][M][ksub] tables -> the reference's `luts` (sample * ksub rows, M columns)."""
    s, M, ksub = lut_sample.shape
    return np.ascontiguousarray(lut_sample.transpose(0, 2, 1).reshape(s * ksub, M))


def sample_rows(n: int, ratio: float) -> np.ndarray:
    """The rows learnQuantization takes: the first int(ratio * float(n)) of randomPermutation."""
    size = int(np.float32(ratio) * np.float32(n))
    return random_permutation(n)[:size]
