"""BitVecEngine::queryLUT's top k with its own tie order (BitVecEngine.hpp:1282-1317), restated in Python, and
the inputs of the fixtures under tests/golden/seq_exact/ (regenerated here from a seed; the fixtures hold the
outputs of the loop run over the real libstdc++ heap functions, and a digest of these inputs).

The loop keeps its k best in a std::vector under std::push_heap / std::pop_heap / std::sort_heap with the
comparator a.dist < b.dist: bits/stl_heap.h's __push_heap and __adjust_heap, restated below as they are in
vaq_amd/csrc/vaq_restated.h (namespace stdheap)."""
import hashlib
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_exact")
FLT_MAX = float(np.finfo(np.float32).max)

# name -> (bits per dimension, centroids and queries on a small integer grid?)
CASES = {
    "grid_d4": ([1, 1, 2, 1], True),         # sums are small integers: nearly every row ties with others
    "grid_d6": ([3, 2, 2, 1, 1, 1], True),
    "cont_d5": ([8, 5, 3, 6, 2], False),     # odd M, continuous centroids: few ties (duplicated rows only)
}
TIE_HEAVY = ("grid_d4", "grid_d6")
N_ROWS = 3000
N_QUERIES = 33
KS = (1, 7, 100)


def row_counts(k):
    return (k - 1, k, k + 1, 300, 3000)


def make_inputs(name):
    """(bits, cent 256 x ndim float32 -- column d holds the 1 << bits[d] centroids of dimension d --, codes
    N_ROWS x ndim uint16, X N_QUERIES x ndim float32) of a case, from its fixed seed."""
    bits, grid = CASES[name]
    ndim = len(bits)
    rng = np.random.default_rng(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    cent = np.zeros((256, ndim), np.float32)
    for d, b in enumerate(bits):
        n = 1 << b
        if grid:
            cent[:n, d] = np.sort(rng.choice(np.arange(-6, 7), size=n, replace=False)).astype(np.float32)
        else:
            cent[:n, d] = np.sort(rng.normal(size=n) * 20).astype(np.float32)
    codes = np.stack([rng.integers(0, 1 << b, N_ROWS) for b in bits], 1).astype(np.uint16)
    if grid:
        X = rng.integers(-7, 8, size=(N_QUERIES, ndim)).astype(np.float32)
        codes[1] = codes[0]  # k = 1 keeps row 1 of two equal first rows: the pop takes the heap's front
    else:
        X = (rng.normal(size=(N_QUERIES, ndim)) * 20).astype(np.float32)
        codes[1500:1506] = codes[:6]  # a few exact duplicates: a few queries tie
        codes[200:203] = codes[10:13]
    return list(bits), cent, codes, X


def digest(bits, cent, codes, X):
    h = hashlib.sha256()
    for a in (np.asarray(bits, np.int32), cent, codes, X):
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def load_fixture(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def centroid_list(bits, cent):
    """the centroids as VaqHip.mCentroidsPerSubs takes them"""
    return [np.ascontiguousarray(cent[: 1 << b, d:d + 1]) for d, b in enumerate(bits)]


def row_dists(xq, bits, cent, codes):
    """float32 [N]: dist = 0; dist += lut[col][code] column by column (BitVecEngine.hpp:1295-1300), with
    lut[col][c] = (x - centroid)^2 in float32 (:1253-1254, :1265-1266)."""
    acc = np.zeros(codes.shape[0], np.float32)
    for d, b in enumerate(bits):
        diff = (np.float32(xq[d]) - cent[: 1 << b, d]).astype(np.float32)
        lut = (diff * diff).astype(np.float32)
        acc = (acc + lut[codes[:, d]]).astype(np.float32)
    return acc


# ---- bits/stl_heap.h over a list of (dist, idx), compared by dist alone ----
def _sift_up(h, hole, top, v):  # std::__push_heap
    parent = (hole - 1) // 2
    while hole > top and h[parent][0] < v[0]:
        h[hole] = h[parent]
        hole = parent
        parent = (hole - 1) // 2
    h[hole] = v


def _adjust_heap(h, hole, length, v):  # std::__adjust_heap
    top = hole
    second = hole
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if h[second][0] < h[second - 1][0]:
            second -= 1
        h[hole] = h[second]
        hole = second
    if length % 2 == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        h[hole] = h[second - 1]
        hole = second - 1
    _sift_up(h, hole, top, v)


def push_heap(h):
    """std::push_heap(h.begin(), h.end()): the new element is the last one"""
    _sift_up(h, len(h) - 1, 0, h[-1])


def _pop_to(h, last):  # std::__pop_heap(first, last, last)
    v = h[last]
    h[last] = h[0]
    _adjust_heap(h, 0, last, v)


def pop_heap(h):
    """std::pop_heap(h.begin(), h.end()): the maximum goes to the last slot"""
    if len(h) > 1:
        _pop_to(h, len(h) - 1)


def sort_heap(h):
    last = len(h)
    while last > 1:
        last -= 1
        _pop_to(h, last)


def query_lut_topk(dists, k):
    """The loop of BitVecEngine.hpp:1287-1316 over one query's row distances (finite): labels and distances,
    k slots each, unfilled ones -1 / FLT_MAX."""
    pairs = []
    bsf = FLT_MAX
    for i, dist in enumerate(np.asarray(dists, np.float32).tolist()):
        if dist < bsf:
            pairs.append((dist, i))
            push_heap(pairs)
            if i >= k:
                pop_heap(pairs)
                pairs.pop()
                bsf = pairs[0][0]
    sort_heap(pairs)
    lab = np.full(k, -1, np.int32)
    dis = np.full(k, FLT_MAX, np.float32)
    lab[: len(pairs)] = [p[1] for p in pairs]
    dis[: len(pairs)] = [p[0] for p in pairs]
    return lab, dis


def smallest_label_topk(dists, k):
    """the scan's own rule: the k smallest (distance, row) pairs"""
    d = np.asarray(dists, np.float32)
    order = np.lexsort((np.arange(d.size), d))[:k]
    lab = np.full(k, -1, np.int32)
    dis = np.full(k, FLT_MAX, np.float32)
    lab[: order.size] = order
    dis[: order.size] = d[order]
    return lab, dis
