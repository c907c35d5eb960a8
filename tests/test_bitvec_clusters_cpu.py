"""The checker of the cluster form (tests/bitvec_clusters_ref.py) on an input worked out by hand, and the refusals the
adapter makes before the library is touched.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import bitvec_clusters_ref as cr
import vaq_amd


def test_checker_on_a_worked_example():
    """Six rows of one word, query 0, so a row's distance is its popcount:

        row      0  1  2  3  4  5
        bits     3  1  7  1  0  3      distance 2  1  3  1  0  2
        cluster  1  0  1  0  1  0      cluster 0 = rows {1, 3, 5}, cluster 1 = rows {0, 2, 4}

    The original query (0) is nearer to centre 0 (at 1, distance 1) than to centre 1 (at 3, distance 9).

    k = 2, atleast 1: cluster 0 alone holds k rows.  Candidates 1, 3, 5 with distances 1, 1, 2; the head (1, 3) is
    sorted, 5 is not smaller than the last: rows 1, 3.
    k = 2, atleast 2: candidates 1, 3, 5, 0, 2, 4 with distances 1, 1, 2, 2, 3, 0.  Row 4 (distance 0) replaces the
    last of the head and moves to the front: rows 4, 1 -- row 3, equal to row 1, is the one pushed out.
    k = 3, atleast 1: the head is (1, 3, 5) = distances 1, 1, 2; nothing follows: rows 1, 3, 5.
    k = 3, atleast 2: head as before; row 0 (distance 2) ties with the last, row 5, across the cut and stays out;
    row 4 (distance 0) pushes row 5 out: rows 4, 1, 3."""
    rows = np.array([[3], [1], [7], [1], [0], [3]], np.uint64)
    queries = np.zeros((1, 1), np.uint64)
    cen = np.array([[1.0], [3.0]], np.float32)
    idx = np.array([1, 0, 1, 0, 1, 0], np.int32)
    oq = np.zeros((1, 1), np.float32)
    for k, atleast, labels, dists in [(2, 1, [1, 3], [1, 1]), (2, 2, [4, 1], [0, 1]), (3, 1, [1, 3, 5], [1, 1, 2]),
                                      (3, 2, [4, 1, 3], [0, 1, 1])]:
        lab, dis = cr.query_clusters(rows, queries, cen, idx, oq, k, atleast, id_base=10)
        assert lab.tolist() == [[10 + r for r in labels]] and dis.tolist() == [dists], (k, atleast)
    # fewer candidates than k: the slots behind them are empty
    lab, dis = cr.query_clusters(rows, queries, cen, idx, oq, 8, 1)
    assert lab.tolist() == [[4, 1, 3, 5, 0, 2, -1, -1]] and dis[0, 6:].tolist() == [0xffffffff] * 2
    # the rerank form: kTemp = 4 candidates (4, 1, 3, then 5 ahead of its equal 0), reranked by |x - 0|^2
    X = np.array([[9], [2], [9], [1], [3], [1]], np.uint8)
    lab, dis = cr.query_rerank_clusters(rows, queries, cen, idx, X, oq, 2, 2, 2)
    assert lab.tolist() == [[3, 5]] and dis.tolist() == [[1.0, 1.0]]


def test_adapter_refuses_before_the_library():
    bv = vaq_amd.VaqBitVec.__new__(vaq_amd.VaqBitVec)  # (no handle: the refusals come before it is read)
    bv._h, bv.device, bv.n_bits, bv.W = C.c_void_p(), 0, 64, 1
    Q = np.zeros((2, 1), np.uint64)
    calls = [
        lambda: bv.set_clusters(np.zeros(4, np.float32), np.zeros(3, np.int32)),            # centres not T x D
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.zeros(3, np.float32)),     # indices not integers
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.zeros((3, 1), np.int32)),  # not one-dimensional
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.array([0, 2, 1])),         # past the centres
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.array([0, -1, 1])),
    ]
    for call in calls:
        with pytest.raises(vaq_amd.VaqHipError) as e:
            call()
        assert e.value.code == -1
    with pytest.raises(vaq_amd.VaqHipError) as e:  # no cluster state yet
        bv.query_clusters(Q, np.zeros((2, 4), np.float32), 3)
    assert e.value.code == -7
    bv.cluster_D = 4
    for oq in (np.zeros((2, 5), np.float32), np.zeros((3, 4), np.float32)):  # another dimension, another count
        with pytest.raises(vaq_amd.VaqHipError) as e:
            bv.query_clusters(Q, oq, 3)
        assert e.value.code == -1
        with pytest.raises(vaq_amd.VaqHipError) as e:
            bv.query_rerank_clusters(Q, oq, 3, 2, None)
        assert e.value.code == -1
