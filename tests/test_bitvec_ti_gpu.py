"""VaqBitVec.query_naive_ti on the GPU against tests/bitvec_ti_ref.py (the k smallest of all rows by (distance, row)),
labels and distances array_equal.  The kernel walks tiles of 256 positions in chunks of 32 dimensions, cuts every cluster
to the annulus of the present threshold before it loads a row, and keeps its candidates in a pool of 2048 keys."""
import numpy as np
import pytest

import bitvec_ti_ref as tr
from vaq_amd import QueryMethod, VaqBitVec, VaqRefiner

pytestmark = pytest.mark.gpu
f32 = np.float32


def build(X, cen, as_bytes=False, id_base=0):
    bv = VaqBitVec(0, 64)  # the bits are never read
    bv.set_rows(np.zeros((len(X), 1), np.uint64), id_base=id_base)
    r = VaqRefiner(X.shape[1], 0)
    (r.set_rows_u8 if as_bytes else r.set_rows)(X.astype(np.uint8 if as_bytes else np.float32), id_base=id_base)
    bv.set_ti_clusters_from_refiner(cen, r)
    return bv, r


def check(X, cen, XQ, k, id_base=0, forms=(False,), refresh=None):
    want = tr.query_naive_ti(X, XQ, k, id_base)
    for as_bytes in forms:
        bv, r = build(X, cen, as_bytes, id_base)
        if refresh:
            bv.set_option("ti_refresh", refresh)
        lab, dis, ev = bv.query_naive_ti(XQ, k, r, evaluated=True)
        r.close()
        bv.close()
        assert np.array_equal(lab, want[0]) and np.array_equal(dis, want[1]), as_bytes
        assert (ev >= min(k, len(X))).all() and (ev <= len(X)).all()
    return ev


# element loads, the chunk seam, aligned pieces past one chunk (40), the refiner's widest row; small integers, so every
# cut falls in a crowd of equal distances
@pytest.mark.parametrize("D", [1, 5, 31, 32, 33, 40, 67, 8176])
def test_widths_and_loads(vaqlib, D):
    rs = np.random.RandomState(D)
    check(rs.randint(0, 4, (1200, D)), rs.randint(0, 4, (7, D)).astype(f32) + f32(0.25),
          rs.randint(0, 4, (9, D)).astype(f32), 17, id_base=1000, forms=(False, True))


@pytest.mark.parametrize("n,k", [(300, 1), (300, 299), (300, 300), (300, 305), (3000, 1024)])
def test_k_edges(vaqlib, n, k):
    rs = np.random.RandomState(n + k)
    check(rs.randint(0, 6, (n, 6)), rs.randint(0, 6, (5, 6)).astype(f32), rs.randint(0, 6, (4, 6)).astype(f32), k)


# one centre; mostly empty clusters; sizes [600, 0, 1, 257, 100, 200, 42]: a cluster above two tiles, ranges across seams
@pytest.mark.parametrize("shape", ["T1", "T4096", "sizes"])
def test_cluster_shapes(vaqlib, shape):
    rs = np.random.RandomState(11)
    if shape == "sizes":
        sizes = [600, 0, 1, 257, 100, 200, 42]
        cen = (np.arange(7)[:, None] * 10 + np.zeros((7, 4))).astype(f32)
        cen[1] = 1000  # no row is nearest to it
        X = np.repeat(cen, sizes, axis=0) + rs.randint(-2, 3, (1200, 4))
        X = X[rs.permutation(1200)].astype(f32)
        XQ = (cen[[0, 3, 4, 6]] + rs.randint(-3, 4, (4, 4))).astype(f32)
    else:
        X = rs.randint(0, 8, (1200, 4))
        cen = rs.uniform(0, 8, (1 if shape == "T1" else 4096, 4)).astype(f32)
        XQ = rs.randint(0, 8, (4, 4)).astype(f32)
    check(X, cen, XQ, 17)


def test_real_valued_data(vaqlib):  # nothing is a tie here: equality with the reference is what the slack protects
    rs = np.random.RandomState(24)
    cen = (3 * rs.standard_normal((20, 24))).astype(f32)
    X = (cen[rs.randint(0, 20, 5000)] + rs.standard_normal((5000, 24))).astype(f32)
    XQ = (cen[rs.randint(0, 20, 16)] + rs.standard_normal((16, 24))).astype(f32)
    ev = check(X, cen, XQ, 100)
    assert ev.mean() < 5000  # (20 separated clusters: some row is out of reach of some query)


# far-first order, the query at the centre: every row is closer than all before it and is admitted.  2048: the pool is
# compacted by its overflow alone; 64: after every tile
@pytest.mark.parametrize("refresh", [64, 2048])
def test_pool_overflow(vaqlib, refresh):
    X = np.zeros((5000, 2), f32)
    X[:, 0] = np.random.RandomState(5).permutation(5000) + 1
    ev = check(X, np.zeros((1, 2), f32), np.zeros((1, 2), f32), 100, refresh=refresh)
    assert ev[0] == 5000


def test_pruning_happens(vaqlib):  # a condition, not a measurement: every other cluster is 98 away, the threshold below 2
    rs = np.random.RandomState(6)
    k, sizes = 10, rs.randint(10, 40, 16)
    cen = np.array([[100 * i, 100 * j, 0] for i in range(4) for j in range(4)], f32)
    X = (np.repeat(cen, sizes, axis=0) + rs.uniform(-0.5, 0.5, (sizes.sum(), 3))).astype(f32)
    near = rs.randint(0, 16, 12)
    XQ = (cen[near] + rs.uniform(-0.5, 0.5, (12, 3))).astype(f32)
    ev = check(X, cen, XQ, k)
    assert (ev >= k).all() and (ev <= sizes[near]).all(), (ev, sizes[near])


def test_unslacked_bound_would_lose_a_neighbour(vaqlib):
    """c1, x and q lie on the first axis, where the sums are one-dimensional: qcc = 1.3376621, xcc = 0.23548116, d(q, x) =
    1.1021808, fl(qcc - xcc) = 1.10218096, one ulp more.  On that axis no y can sit at exactly that distance in a cluster
    of its own (beyond q the spacing of the floats skips it, before q it falls into x's cluster), so y leaves the axis."""
    c1, x, q = [0.11916632205247879, 0], [-0.1163148358464241, 0], [-1.2184957265853882, 0]
    y, c2 = [-0.7550274133682251, 1], [-0.75, 1]
    d = lambda a, b: tr.dists(np.array(a, f32), np.array([b], f32))[0]
    qcc, xcc = d(q, c1), d(x, c1)
    assert (qcc, xcc, d(q, x), f32(qcc - xcc)) == (f32(1.3376621), f32(0.23548116), f32(1.1021808), f32(1.10218096))
    assert d(q, x) < d(q, y) and d(q, y) <= f32(qcc - xcc)  # the reference's `bsfK <= qToCC - dToCC` would skip x
    assert d(q, c2) < qcc and d(y, c2) < d(y, c1) and d(x, c1) < d(x, c2)  # y's cluster is visited first
    X, cen, XQ = np.array([y, x], f32), np.array([c1, c2], f32), np.array([q], f32)
    bv, r = build(X, cen)
    lab, dis = bv.query_naive_ti(XQ, 1, r)
    assert lab[0, 0] == 1 and dis[0, 0] == d(q, x)
    r.close()
    bv.close()


def test_state(vaqlib):
    rs = np.random.RandomState(8)
    X, cen, XQ = rs.randint(0, 4, (300, 3)), rs.uniform(0, 4, (4, 3)).astype(f32), rs.randint(0, 4, (2, 3)).astype(f32)
    bv = VaqBitVec(0, 64)
    bv.set_rows(np.zeros((300, 1), np.uint64))
    r = VaqRefiner(3, 0)
    r.set_rows(X.astype(f32))
    lab, dis = np.empty((2, 3), np.int32), np.empty((2, 3), f32)

    def raw(nq=2):  # the C entry itself
        return vaqlib.vaqhip_bitvec_query_naive_ti(bv._h, r._h, XQ.ctypes.data, nq, 3, QueryMethod.Heap, lab.ctypes.data,
                                                   dis.ctypes.data, None)
    assert raw() == -7  # before the build
    idx = r.cluster_index(cen)
    bv.set_clusters(cen, idx)
    before = bv.query_naive_clusters(XQ, 3, r, atleast_cluster=2)
    bv.set_ti_clusters_from_refiner(cen, r)
    assert raw(nq=0) == 0 and raw() == 0
    after = bv.query_naive_clusters(XQ, 3, r, atleast_cluster=2)  # both states exist at once
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(lab, tr.query_naive_ti(X, XQ, 3)[0])
    bv.set_rows(np.zeros((300, 1), np.uint64))  # the rows change: both states go
    assert raw() == -7
    r.close()
    bv.close()
