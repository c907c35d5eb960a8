"""FAST across the shards of a multi-device index, the part that needs no GPU: the rule of DESIGN.md section 4c
("FAST across shards") restated in NumPy (tests/fast_multi_ref.py) equals KNNFromDists over the whole distance
array (tests/fast_ref.py, pinned to the reference by tests/golden/fast/), slot for slot; the design that lets a
shard truncate head rows does not; and the library exports the new entry points and checks their arguments."""
import ctypes as C

import numpy as np
import pytest

import fast_multi_ref as fm
import fast_ref as fr

GS = [1, 2, 3, 8, 16]
KS = [1, 16, 17, 100, 1024]


def dists(rng, n, distinct):
    """uint16 distances over `distinct` values: 2 = ties everywhere, 8 = at the cut, 4096 = rare"""
    return rng.integers(0, distinct, size=n).astype(np.uint16).astype(np.int64) * (32640 // distinct)


def sizes(G, k):
    """N from below k to well above G * k; shards without rows (N < G) among them"""
    return sorted({1, 2, max(1, G - 1), max(1, k // 2), k, k + 1, k + G, 2 * k + 3, G * max(1, 3 * k // 4), G * k,
                   G * k + 37, 3 * G * k + 5})


def head_span(bounds, kk):
    return sum(1 for lo, hi in bounds if min(hi, kk) > min(lo, kk))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("G", GS)
def test_rule_equals_knn_from_dists(G, k):
    rng = np.random.default_rng(1000 * G + k)
    spans, empties, whole = set(), 0, False
    for N in sizes(G, k):
        bounds = fm.shard_bounds(N, G)
        assert bounds[0][0] == 0 and bounds[-1][1] == N and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
        spans.add(head_span(bounds, min(k, N)))
        whole = whole or head_span(bounds, min(k, N)) == sum(1 for lo, hi in bounds if hi > lo) > 1
        empties += sum(1 for lo, hi in bounds if hi == lo)
        for distinct in (2, 8, 4096):
            d = dists(rng, N, distinct)
            el, ed = fr.knn_from_dists(d, k)
            gl, gd = fm.search(d, bounds, k)
            assert np.array_equal(gl, el) and np.array_equal(gd, ed), (G, k, N, distinct)
    # the head lay in one shard, in two, and in every shard that has rows; some shards had no rows
    assert 1 in spans
    if G > 1 and k >= 16:
        assert 2 in spans and whole
    if G > 2:
        assert empties > 0


@pytest.mark.parametrize("G,k,first,adds", [(3, 17, 10, [4, 30]), (8, 100, 60, [39, 1, 500]), (2, 16, 40, [7, 7])])
def test_rule_after_appends(G, k, first, adds):
    """appended rows extend the LAST shard: the bounds are no longer ceil(N / G) each, and the head may grow"""
    rng = np.random.default_rng(77 + G)
    bounds = fm.shard_bounds(first, G)
    N = first
    for a in adds:
        N += a
        bounds[-1] = (bounds[-1][0], N)
        for distinct in (2, 8, 4096):
            d = dists(rng, N, distinct)
            el, ed = fr.knn_from_dists(d, k)
            gl, gd = fm.search(d, bounds, k)
            assert np.array_equal(gl, el) and np.array_equal(gd, ed), (G, k, N, distinct)


def test_truncating_head_rows_is_wrong():
    """Two shards of 32 rows, k = 20.  The head (rows 0..19) ties at distance 5, twelve more rows of shard 0 lie
    below it and everything else above: the k-th distance is 5, shard 0 holds 32 > k rows at or below it, and
    its plain top-k by (dist, row) keeps head rows 0..7 -- but which eight head rows the single index returns is
    decided by std::sort's permutation of the twenty, which is not the row order."""
    k, N = 20, 64
    d = np.full(N, 9, np.int64)
    d[:20] = 5
    d[20:32] = 1
    bounds = fm.shard_bounds(N, 2)
    assert bounds == [(0, 32), (32, 64)]
    el, ed = fr.knn_from_dists(d, k)
    assert ed[k - 1] == 5 and int(np.sum(d[:32] <= 5)) > k
    assert set(el[12:].tolist()) != set(range(8))          # the case does what it was built for
    gl, gd = fm.search(d, bounds, k)
    assert np.array_equal(gl, el) and np.array_equal(gd, ed)
    tl, td = fm.truncating(d, bounds, k)
    assert np.array_equal(td, ed)                           # the distances alone would not show it
    assert not np.array_equal(tl, el)


def test_merge_of_hand_built_lists():
    """ties between the head and two lists, and inside the head: the head first, then the earlier list"""
    head = np.array([7, 3, 7, 3], np.int64)                 # rows 0..3
    lists = [(np.array([5, 4, 6]), np.array([3, 7, 7])), (np.array([9, 8]), np.array([3, 8]))]
    lab, dis = fm.merge(head, lists, 8)
    assert lab.tolist() == [1, 3, 5, 9, 0, 2, 4, 6]
    assert dis.tolist() == [3, 3, 3, 3, 7, 7, 7, 7]
    lab, dis = fm.merge(head[:2], [(np.array([], np.int64), np.array([], np.int64))], 4)
    assert lab.tolist() == [1, 0, -1, -1] and dis[2] == fm.FLT_MAX


# ------------------------------------------------------------------------------------ the C ABI
def test_new_entry_points_are_exported(vaqlib):
    for name in ("vaqhip_multi_set_lut_quantization", "vaqhip_multi_learn_quantization", "vaqhip_merge_fast_device"):
        assert hasattr(vaqlib, name), name
    assert vaqlib.vaqhip_version() >= 106


def test_merge_fast_argument_validation(vaqlib):
    """refused before any device is touched: EINVAL (-1) / EUNSUPPORTED (-2)"""
    f = vaqlib.vaqhip_merge_fast_device
    p = C.c_void_p(64)  # never dereferenced on these paths
    nq, k = 4, 10

    def call(head=p, n_head=k, dist=p, lab=p, n_lists=2, out_l=p, out_d=p, k=k, head_stride=None):
        return f(0, head, k if head_stride is None else head_stride, n_head, 0, dist, lab, n_lists, nq * k, k, nq, k,
                 out_l, out_d, None)
    assert call(head=None) == -1
    assert call(dist=None) == -1
    assert call(lab=None) == -1
    assert call(out_l=None) == -1
    assert call(out_d=None) == -1
    assert call(k=1025, n_head=0) == -2 and b"1024" in vaqlib.vaqhip_last_error()
    assert call(n_lists=17) == -2 and b"16" in vaqlib.vaqhip_last_error()
    assert call(k=0) == -1
    assert call(n_head=k + 1) == -1          # the head is at most k rows
    assert call(n_head=k, head_stride=k - 1) == -1
    assert call(n_lists=-1) == -1


def test_multi_quantization_argument_validation(vaqlib):
    one = (C.c_float * 8)(*[1.0] * 8)
    assert vaqlib.vaqhip_multi_set_lut_quantization(None, one, one) == -1
    assert vaqlib.vaqhip_multi_learn_quantization(None, one, 1, 0, C.c_float(0.5), None, None) == -1
    assert b"null" in vaqlib.vaqhip_multi_last_error()
