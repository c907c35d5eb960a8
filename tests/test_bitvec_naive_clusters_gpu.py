"""VaqBitVec.query_naive_clusters on the GPU against tests/bitvec_naive_clusters_ref.py, labels and distances array_equal.
Raw rows are small integers: every cut falls inside a crowd of equal distances that spans the head, the later candidates
and several clusters.  The kernel walks tiles of 256 candidates in chunks of DC = 32 dimensions; its pool has 2048 slots."""
import os
import subprocess

import numpy as np
import pytest

import bitvec_naive_clusters_ref as nr
import bitvec_ref as br
from vaq_amd import QueryMethod, VaqBitVec, VaqRefiner

pytestmark = pytest.mark.gpu
DC = 32
SIZES7 = [600, 0, 1, 257, 100, 200, 42]  # 1200 rows: an empty cluster, one of a single row, one above two tiles


def sizes_to_idx(rs, sizes):
    return rs.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def engine(n, cen, idx, id_base=0):
    bv = VaqBitVec(0, 64)  # the bits are never read
    bv.set_rows(np.zeros((n, 1), np.uint64), id_base=id_base)
    if cen is not None:
        bv.set_clusters(cen, idx)
    return bv


def refiner(X, as_bytes, id_base=0):
    r = VaqRefiner(X.shape[1], 0)
    (r.set_rows_u8 if as_bytes else r.set_rows)(X.astype(np.uint8 if as_bytes else np.float32), id_base=id_base)
    return r


def check(X, cen, idx, XQ, k, atleast=1, id_base=0, forms=(True, False)):
    want = nr.query_naive_clusters(X, cen, idx, XQ, k, atleast, id_base)
    bv = engine(len(X), cen, idx, id_base)
    for as_bytes in forms:
        r = refiner(X, as_bytes, id_base)
        got = bv.query_naive_clusters(XQ, k, r, atleast_cluster=atleast)
        r.close()
        assert np.array_equal(got[0], want[0]), as_bytes
        assert np.array_equal(got[1], want[1]), as_bytes
    bv.close()
    return want


def small_ints(rs, n, D, nq, T):
    return (rs.randint(0, 4, (n, D)), rs.standard_normal((T, D)).astype(np.float32),
            rs.randint(0, 4, (nq, D)).astype(np.float32))


# element loads, the chunk seam, aligned pieces past one chunk (40), the refiner's widest row (the chunk loop bounds LDS)
@pytest.mark.parametrize("D", [1, 5, DC - 1, DC, DC + 1, 2 * DC + 3, 40, 8176])
def test_widths_and_loads(vaqlib, D):
    rs = np.random.RandomState(D)
    X, cen, XQ = small_ints(rs, 1200, D, 9, 7)
    check(X, cen, sizes_to_idx(rs, SIZES7), XQ, 17, 1, id_base=1000)


@pytest.mark.parametrize("atleast", [1, 3, 7])
def test_atleast_cluster(vaqlib, atleast):
    rs = np.random.RandomState(7)
    X, cen, XQ = small_ints(rs, 1200, 5, 9, 7)
    want = check(X, cen, sizes_to_idx(rs, SIZES7), XQ, 17, atleast)
    if atleast == 7:  # every row is visited: the distances of the exhaustive composition
        for q in range(9):
            assert np.array_equal(want[1][q], np.sort(br.euclidean_no_sqrt(XQ[q], X))[:17])


# a head of four tiles whose last tile's tail is admitted by threshold; of one tile and one row more; n < k
@pytest.mark.parametrize("n,k,sizes", [(1100, 1024, [500, 300, 300]), (1100, 256, [500, 300, 300]),
                                       (1100, 257, [500, 300, 300]), (700, 1024, [400, 0, 300])])
def test_head_edges(vaqlib, n, k, sizes):
    rs = np.random.RandomState(n + k)
    X, cen, XQ = small_ints(rs, n, 8, 4, len(sizes))
    check(X, cen, sizes_to_idx(rs, sizes), XQ, k, len(sizes))


@pytest.mark.parametrize("n,k", [(3000, 100), (3000, 1000), (5000, 100)])
@pytest.mark.parametrize("order", ["ramp", "flat"])
def test_compaction(vaqlib, order, n, k):
    # ramp: distances fall for query 0 (all admitted; at k = 1000 compacted from exactly 2048 slots), rise for query 1
    X = np.zeros((n, 2), np.float32)
    XQ = np.array([[0, 1], [n + 1, 1]], np.float32)
    if order == "ramp":
        X[:, 0] = n - np.arange(n)  # (squares of integers: adjacent ones stay apart in float32 far past 5001^2)
    want = check(X, np.zeros((1, 2), np.float32), np.zeros(n, np.int32), XQ, k,
                 forms=(True, False) if order == "flat" else (False,))
    if order == "ramp":
        assert np.array_equal(want[0][0], np.arange(n - 1, n - 1 - k, -1)) and np.array_equal(want[0][1], np.arange(k))


def test_infinite_distances(vaqlib):  # finite rows at +-3e19 overflow: slot k inside the run of infinities
    rs = np.random.RandomState(3)
    X, cen, XQ = small_ints(rs, 600, 4, 3, 3)
    X = X.astype(np.float32)
    X[:, 0] = np.where(rs.randint(0, 2, 600) == 1, 3e19, -3e19)
    XQ[:, 0] = 3e19
    want = check(X, cen, sizes_to_idx(rs, [250, 150, 200]), XQ, 400, 3, id_base=9, forms=(False,))
    assert (want[0] >= 9).all() and np.isinf(want[1][:, -1]).all() and np.isfinite(want[1][:, 0]).all()


def test_float_only_arithmetic(vaqlib):
    rs = np.random.RandomState(37)
    X = rs.standard_normal((1200, 37)).astype(np.float32)
    XQ = rs.standard_normal((5, 37)).astype(np.float32)
    cen = rs.standard_normal((7, 37)).astype(np.float32)
    want = check(X, cen, sizes_to_idx(rs, SIZES7), XQ, 17, 7, forms=(False,))
    d64 = ((XQ[:, None, :].astype(np.float64) - X[None]) ** 2).sum(axis=2).astype(np.float32)
    assert not np.array_equal(np.sort(d64, axis=1)[:, :17], want[1])  # a sum kept wider would answer otherwise


@pytest.mark.parametrize("case,code", [("method_heap", -2), ("atleast_0", -1), ("atleast_T_plus_1", -1),
                                       ("refiner_D", -1), ("refiner_rows", -7), ("before_set_clusters", -7)])
def test_refusals(vaqlib, case, code):
    rs = np.random.RandomState(9)
    X, cen, XQ = small_ints(rs, 300, 3, 2, 4)
    bv = engine(300, None if case == "before_set_clusters" else cen, rs.randint(0, 4, 300).astype(np.int32))
    r = refiner({"refiner_D": X[:, :2], "refiner_rows": X[:299]}.get(case, X), True)
    lab, dis = np.empty((2, 3), np.int32), np.empty((2, 3), np.float32)

    def raw(method=QueryMethod.Sort, atleast=1):  # the C entry itself: the adapter's own refusals are not in the way
        return vaqlib.vaqhip_bitvec_query_naive_clusters(bv._h, r._h, XQ.ctypes.data, 2, 3, method, atleast, lab.ctypes.data,
                                                         dis.ctypes.data)
    assert raw(**{"method_heap": dict(method=QueryMethod.Heap), "atleast_0": dict(atleast=0),
                  "atleast_T_plus_1": dict(atleast=5)}.get(case, {})) == code
    r.close()
    bv.close()


def test_device_form_on_two_streams(vaqlib):  # nothing synchronised until both calls are enqueued
    import torch
    rs = np.random.RandomState(5)
    X, cen, _ = small_ints(rs, 1200, 8, 1, 7)
    idx = sizes_to_idx(rs, SIZES7)
    calls = [(rs.randint(0, 4, (9, 8)).astype(np.float32), 17), (rs.randint(0, 4, (70, 8)).astype(np.float32), 300)]
    bv, r = engine(1200, cen, idx), refiner(X, True)
    dev = [torch.from_numpy(xq).cuda() for xq, _ in calls]
    torch.cuda.synchronize()
    streams, out = [torch.cuda.Stream(), torch.cuda.Stream()], [None, None]
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            out[i] = bv.query_naive_clusters_device(dev[i], calls[i][1], r, atleast_cluster=2)
    torch.cuda.synchronize()
    for (xq, k), got in zip(calls, out):
        want = nr.query_naive_clusters(X, cen, idx, xq, k, 2)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    r.close()
    bv.close()


def test_cpp_shim(vaqlib, tmp_path):  # tests/cpp/bitvec_naive_shim_test.cpp reads the inputs and the restatement's answers
    from vaq_amd import build
    rs = np.random.RandomState(12)
    n, nq, D, T, k, atleast = 400, 5, 8, 4, 10, 2
    X, cen, XQ = small_ints(rs, n, D, nq, T)
    idx = rs.randint(0, T, n).astype(np.int32)
    lab, dis = nr.query_naive_clusters(X, cen, idx, XQ, k, atleast)
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([n, nq, D, T, k, atleast], np.int32).tobytes())
        for a in (X.astype(np.uint8), XQ, cen, idx, lab, dis):
            f.write(np.ascontiguousarray(a).tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "bitvec_naive_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "bitvec_naive_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bitvec_naive_shim ok" in out.stdout, out.stdout + out.stderr
