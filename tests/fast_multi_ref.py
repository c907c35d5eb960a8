"""NumPy restatement of FAST across the shards of a multi-device index ("FAST across
shards"), the checker of tests/test_fast_multi_*.py.

The single index returns the k smallest rows by (dist, seq): seq = the position std::sort gives a row of the
head (index positions 0..kk-1, kk = min(k, N)), the row itself after (fast_ref.knn_from_dists).  Put as a
sequence: the first k of a STABLE sort by distance of "the head in std::sort's output order, then every other
row in row order".  Cut into shards of contiguous rows:

  shard_parts   what one shard hands over: the distances of the head rows it holds (all of them), and the top
                min(k, count) of its OTHER rows by (dist, row)
  merge         the head sorted once by std_sort_perm, then the stable merge by distance alone of the head list
                and the shards' lists in shard order, first k
  truncating    the tempting wrong design: every shard's plain top-k by (dist, row) over ALL its rows, so head
                rows can be cut off by their own shard
"""
from __future__ import annotations

import numpy as np

import fast_ref as fr

FLT_MAX = np.finfo(np.float32).max


def shard_bounds(N: int, G: int):
    """vaqhip_multi_set_codes_u16: shard g = rows [g * ceil(N / G), (g + 1) * ceil(N / G)) cut at N."""
    per = (N + G - 1) // G
    return [(min(N, g * per), min(N, (g + 1) * per)) for g in range(G)]


def shard_parts(d: np.ndarray, lo: int, hi: int, k: int):
    """(head positions, head distances, list rows, list distances) of the shard holding rows [lo, hi)."""
    kk = min(k, d.shape[0])
    h_lo, h_hi = min(lo, kk), min(hi, kk)
    rows = np.arange(max(lo, kk), max(hi, kk), dtype=np.int64)
    order = np.lexsort((rows, d[rows]))[:k]
    return np.arange(h_lo, h_hi), d[h_lo:h_hi], rows[order], d[rows[order]]


def merge(head_dist: np.ndarray, lists, k: int):
    """head_dist [kk]; lists: (rows, dists) per shard in shard order.  Returns (labels int64 [k], dists float32 [k])."""
    head = fr.std_sort_perm(head_dist)  # rows of the head in std::sort's output order
    rows = np.concatenate([head] + [r for r, _ in lists]).astype(np.int64)
    dist = np.concatenate([np.asarray(head_dist, np.int64)[head]] + [np.asarray(x, np.int64) for _, x in lists])
    take = np.argsort(dist, kind="stable")[:k]  # ties: the earlier list, then the earlier position
    lab = np.full(k, -1, np.int64)
    dis = np.full(k, FLT_MAX, np.float32)
    lab[:take.shape[0]] = rows[take]
    dis[:take.shape[0]] = dist[take].astype(np.float32)
    return lab, dis


def search(d, bounds, k: int):
    """The rule end to end over the distances d [N] of one query and the shards' row ranges."""
    d = np.asarray(d, np.int64)
    kk = min(k, d.shape[0])
    head = np.zeros(kk, np.int64)
    lists = []
    for lo, hi in bounds:
        pos, hd, rows, ld = shard_parts(d, lo, hi, k)
        head[pos] = hd
        lists.append((rows, ld))
    return merge(head, lists, k)


def truncating(d, bounds, k: int):
    """Every shard keeps its plain top-k by (dist, row) over all its rows; the survivors are then ranked by the
    true (dist, seq) -- as generous to this design as can be."""
    d = np.asarray(d, np.int64)
    n = d.shape[0]
    kk = min(k, n)
    seq = np.arange(n, dtype=np.int64)
    seq[fr.std_sort_perm(d[:kk])] = np.arange(kk)
    keep = []
    for lo, hi in bounds:
        rows = np.arange(lo, hi, dtype=np.int64)
        keep.append(rows[np.lexsort((rows, d[rows]))[:k]])
    keep = np.concatenate(keep)
    take = keep[np.lexsort((seq[keep], d[keep]))[:kk]]
    lab = np.full(k, -1, np.int64)
    dis = np.full(k, FLT_MAX, np.float32)
    lab[:take.shape[0]] = take
    dis[:take.shape[0]] = d[take].astype(np.float32)
    return lab, dis
