"""The cluster index on the GPU (vaq_cluster_index.hip) against tests/cluster_index_ref.py, indices and distances
array_equal.  Rows and centres are small integers and two centres are identical: many rows have several equally near
centres and the first must win.  The kernel owns 256 rows a workgroup, DC = 32 dimensions a chunk, TC = 64 centres a block."""
import os
import subprocess

import numpy as np
import pytest

import bitvec_naive_clusters_ref as nr
import cluster_index_ref as cr
import vaq_amd
from vaq_amd import VaqBitVec, VaqHipError, VaqRefiner

pytestmark = pytest.mark.gpu
DC, TC = 32, 64


def refiner(X, as_bytes):
    r = VaqRefiner(X.shape[1], 0)
    (r.set_rows_u8 if as_bytes else r.set_rows)(X.astype(np.uint8 if as_bytes else np.float32))
    return r


def small_ints(rs, n, D, T):
    X, cen = rs.randint(0, 4, (n, D)), rs.randint(0, 4, (T, D)).astype(np.float32)
    if T > 2:
        cen[2] = cen[0]
    return X, cen


def check(X, cen, forms=(False, True)):
    want = cr.cluster_index(X, cen)
    for as_bytes in forms:
        r = refiner(X, as_bytes)
        got = r.cluster_index(cen, return_dist=True)
        only_idx = r.cluster_index(cen)
        r.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(only_idx, want[0]), as_bytes
    return want


# element loads and aligned pieces, the chunk seam, a tail chunk, the widest row; two full workgroups and a tail
@pytest.mark.parametrize("D", [1, 5, DC - 1, DC, DC + 1, 2 * DC + 3, 8176])
def test_widths(vaqlib, D):
    rs = np.random.RandomState(D)
    check(*small_ints(rs, 600, D, 7))


@pytest.mark.parametrize("T", [1, TC - 1, TC, TC + 1, 2 * TC + 2, 4096])
def test_centre_blocks(vaqlib, T):
    rs = np.random.RandomState(T)
    X, cen = small_ints(rs, 300, 3, T)
    cen += 0.5  # no centre equals a row, but the last one: rows equal to X[5] must find it in the last, partial block
    cen[T - 1] = X[5]
    want = check(X, cen)
    assert (want[0][(X == X[5]).all(axis=1)] == T - 1).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_row_tails(vaqlib, n):
    rs = np.random.RandomState(n)
    check(*small_ints(rs, n, 5, 7))


def test_float_only_arithmetic(vaqlib):
    rs = np.random.RandomState(37)
    X, cen = rs.standard_normal((600, 37)).astype(np.float32), rs.standard_normal((7, 37)).astype(np.float32)
    want = check(X, cen, forms=(False,))
    d64 = ((X[:, None, :].astype(np.float64) - cen[None]) ** 2).sum(axis=2).min(axis=1).astype(np.float32)
    assert not np.array_equal(d64, want[1])  # a sum kept wider, or fused, would answer otherwise


def not_finite_case(rs):
    X, cen = small_ints(rs, 300, 3, 3)
    X = X.astype(np.float32)
    X[0, 1] = np.nan          # a NaN in every sum of the row
    X[1] = 3e19               # 9e38 and 3.6e39 overflow: every distance +inf
    cen[0, 2] = np.nan        # never chosen
    cen[1] = -3e19
    return X, cen


def test_not_finite(vaqlib):
    X, cen = not_finite_case(np.random.RandomState(1))
    idx, dist = check(X, cen, forms=(False,))
    assert idx[0] == -1 and idx[1] == -1 and (idx[2:] == 2).all() and dist[0] == cr.FLT_MAX and dist[1] == cr.FLT_MAX


def test_set_clusters_from_refiner_refuses_minus_one(vaqlib):
    rs = np.random.RandomState(2)
    X, cen = not_finite_case(rs)
    good, bits, Q = rs.randint(0, 4, (300, 3)), rs.randint(0, 2 ** 62, (300, 1)).astype(np.uint64), rs.randint(0, 2 ** 62, (4, 1)).astype(np.uint64)
    XQ = rs.randint(0, 4, (4, 3)).astype(np.float32)
    bv = VaqBitVec(0, 64)
    bv.set_rows(bits)
    r = refiner(good, False)
    bv.set_clusters_from_refiner(np.nan_to_num(cen), r)
    before = bv.query_clusters(Q, XQ, 10, atleast_cluster=2)
    r.set_rows(X)
    with pytest.raises(VaqHipError) as e:
        bv.set_clusters_from_refiner(cen, r)
    assert e.value.code == -1 and "row 0 " in str(e.value)
    after = bv.query_clusters(Q, XQ, 10, atleast_cluster=2)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    r.close()
    bv.close()


@pytest.mark.parametrize("as_bytes", [False, True])
def test_composition(vaqlib, as_bytes):
    rs = np.random.RandomState(8)
    X, cen = small_ints(rs, 1200, 8, 7)
    cen[4] = 100.0  # an empty cluster (and cen[2], behind its equal cen[0], is another)
    idx = cr.cluster_index(X, cen)[0]
    assert not (idx == 4).any() and not (idx == 2).any()
    bits, Q = rs.randint(0, 2 ** 62, (1200, 1)).astype(np.uint64), rs.randint(0, 2 ** 62, (9, 1)).astype(np.uint64)
    XQ = rs.randint(0, 4, (9, 8)).astype(np.float32)
    r = refiner(X, as_bytes)
    answers = []
    for from_refiner in (True, False):
        bv = VaqBitVec(0, 64)
        bv.set_rows(bits)
        bv.set_clusters_from_refiner(cen, r) if from_refiner else bv.set_clusters(cen, idx)
        answers.append(bv.query_clusters(Q, XQ, 17, atleast_cluster=3) + bv.query_naive_clusters(XQ, 17, r, atleast_cluster=3))
        bv.close()
    r.close()
    for a, b in zip(*answers):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("as_bytes", [False, True])
def test_forms_agree(vaqlib, as_bytes):
    import torch
    rs = np.random.RandomState(4)
    X, cen = small_ints(rs, 700, 12, 70)
    want = cr.cluster_index(X, cen)
    Xt = X.astype(np.uint8 if as_bytes else np.float32)
    raw = vaq_amd.cluster_index_u8 if as_bytes else vaq_amd.cluster_index
    r = refiner(X, as_bytes)
    d_X, d_cen = torch.from_numpy(Xt).cuda(), torch.from_numpy(cen).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        on_stream = raw(d_X, d_cen, return_dist=True), r.cluster_index_device(d_cen, return_dist=True)
    torch.cuda.synchronize()
    got = [raw(Xt, cen, return_dist=True)] + [(i.cpu().numpy(), d.cpu().numpy()) for i, d in on_stream]
    r.close()
    for idx, dist in got:
        assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1])


@pytest.mark.parametrize("case,code", [("T_0", -1), ("T_4097", -1), ("null_centres", -1), ("null_out", -1), ("D_mismatch", -1),
                                       ("refiner_rows", -7)])
def test_refusals(vaqlib, case, code):  # the C entries themselves: the adapter's own refusals are not in the way
    rs = np.random.RandomState(9)
    X, cen = small_ints(rs, 300, 3, 4)
    r = refiner(X[:299] if case == "refiner_rows" else X, True)
    out = np.full(300, 77, np.int32)
    if case in ("D_mismatch", "refiner_rows"):
        bv = VaqBitVec(0, 64)
        bv.set_rows(np.zeros((300, 1), np.uint64))
        wide = np.zeros((4, 4), np.float32)
        rc = (vaqlib.vaqhip_bitvec_set_clusters_from_refiner(bv._h, r._h, wide.ctypes.data, 4, 4) if case == "D_mismatch" else
              vaqlib.vaqhip_bitvec_set_clusters_from_refiner(bv._h, r._h, cen.ctypes.data, 4, 3))
        bv.close()
    else:
        T = {"T_0": 0, "T_4097": 4097}.get(case, 4)
        rc = vaqlib.vaqhip_refiner_cluster_index(r._h, None if case == "null_centres" else cen.ctypes.data, T,
                                                 None if case == "null_out" else out.ctypes.data, None)
    r.close()
    assert rc == code and (out == 77).all()


def test_cpp_shim(vaqlib, tmp_path):  # tests/cpp/cluster_index_shim_test.cpp reads the inputs and the restatement's answers
    from vaq_amd import build
    rs = np.random.RandomState(12)
    n, nq, D, T, k = 400, 5, 8, 4, 10
    X, cen = small_ints(rs, n, D, T)
    XQ = rs.randint(0, 4, (nq, D)).astype(np.float32)
    idx = cr.cluster_index(X, cen)[0]
    lab, dis = nr.query_naive_clusters(X, cen, idx, XQ, k, 2)
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([n, nq, D, T, k, 2], np.int32).tobytes())
        for a in (X.astype(np.uint8), XQ, cen, idx, lab, dis):
            f.write(np.ascontiguousarray(a).tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cluster_index_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "cluster_index_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "cluster_index_shim ok" in out.stdout, out.stdout + out.stderr
