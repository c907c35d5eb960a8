"""NumPy restatement of VAQ::learnQuantization's alpha loop (VAQ.cpp:1141-1186) with the loss summed as the library
sums it: per (alpha, column) the float32 squares added one after another in double, in table order (sample major,
centroid minor), then the columns added for s = 0 .. M - 1.  The checker of tests/test_learn_device_*.py; the
percentile is tests/fast_ref.py's, which tests/golden/fast/ pins to the reference's own."""
from __future__ import annotations

import numpy as np

import fast_ref as fr


def sequential_sum(terms32: np.ndarray) -> float:
    """l = 0.0; for t in terms: l += (double)t -- np.add.accumulate adds in order, np.sum would add pairwise"""
    t = np.asarray(terms32, np.float32)
    if t.size == 0:
        return 0.0
    return float(np.add.accumulate(t, dtype=np.float64)[-1])


def column_terms(col: np.ndarray, fl: np.float32, sc: np.float32) -> np.ndarray:
    """(ideal * ideal) of VAQ.cpp:1171-1176 for every value of a column, float32 step by step"""
    col = np.asarray(col, np.float32)
    with np.errstate(all="ignore"):
        off = np.maximum(col - fl, np.float32(0))
        qv = np.minimum(np.floor((off * sc).astype(np.float32)), np.float32(255))
        quant = qv.astype(np.int32).astype(np.uint8).astype(np.float32)  # truncated to an int, the low byte kept
        ideal = ((col - off) * sc).astype(np.float32) - quant
        return (ideal * ideal).astype(np.float32)


def learn(lut_sample: np.ndarray):
    """lut_sample [sample][M][ksub] (VaqHip.build_lut of the sampled rows, in sample order).
    Returns (offsets [M], scale [M], alpha index or -1, loss [7] float64, every alpha's scales [7][M])."""
    luts = fr.stack_luts(np.asarray(lut_sample, np.float32))  # (sample * ksub, M): a column in table order
    M = luts.shape[1]
    floors = np.empty((7, M), np.float32)
    scales = np.empty((7, M), np.float32)
    loss = np.zeros(7, np.float64)
    srt = np.sort(luts, axis=0)
    with np.errstate(all="ignore"):
        for ai, a in enumerate(fr.ALPHAS):
            total = 0.0
            for s in range(M):
                fl = fr.percentile(srt[:, s], a)
                ceil = fr.percentile(np.maximum(srt[:, s] - fl, np.float32(0)), np.float32(np.float32(1) - a))
                sc = np.float32(np.float32(255) / ceil)
                floors[ai, s], scales[ai, s] = fl, sc
                total += sequential_sum(column_terms(luts[:, s], fl, sc))
            loss[ai] = total
    best, best_a = float(np.finfo(np.float32).max), -1
    for ai in range(7):
        if loss[ai] <= best:
            best, best_a = loss[ai], ai
    if best_a < 0:
        return None, None, -1, loss, scales
    return floors[best_a], scales[best_a], best_a, loss, scales
