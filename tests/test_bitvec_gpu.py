"""The Hamming engine on the GPU (vaq_amd.VaqBitVec over vaqhip_bitvec_*): BitVecEngine::query and ::queryRerank with
QueryMethod::Sort, label for label and distance for distance against the fixtures the compiled reference recorded
(tests/golden/hamming) and against the restatement (tests/bitvec_ref.py) on random bits.

Shapes: the scan's row tile is 512 rows (256 threads, two rows each) and its query tile 64 queries; rows are padded
to 32; the selection's head is the first min(k, n) rows.  Random rows are full 64-bit words, so wherever n_bits is
no multiple of 64 the tail bits hold noise, and the restatement counts them."""
import glob
import os

import numpy as np
import pytest

import bitvec_ref as br
from vaq_amd import QueryMethod, VaqBitVec, VaqHipError, VaqRefiner

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "hamming")


def words(rs, n, W):
    """n random rows of W full 64-bit words"""
    return rs.randint(0, 1 << 32, (n, W), dtype=np.uint64) | (rs.randint(0, 1 << 32, (n, W), dtype=np.uint64) << np.uint64(32))


def near(rs, centre, n, flip):
    """n rows around one centre row with `flip` random bits turned: small distances with many ties"""
    W = centre.shape[0]
    rows = np.repeat(centre[None, :], n, axis=0).copy()
    for r in range(n):
        for b in rs.randint(0, 64 * W, flip):
            rows[r, b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return rows


def fixtures(prefix):
    return [pytest.param(f, id=os.path.basename(f)[:-4]) for f in sorted(glob.glob(os.path.join(GOLD, prefix + "*.npz")))]


@pytest.mark.parametrize("path", fixtures("hamming_"))
def test_query_matches_reference_fixture(vaqlib, path):
    g = np.load(path)
    bv = VaqBitVec(0, int(g["n_bits"]))
    bv.set_rows(g["rows"])
    lab, dis = bv.query(g["queries"], int(g["k"]))
    assert np.array_equal(lab, g["labels"])
    assert np.array_equal(dis, g["dists"])
    bv.close()


@pytest.mark.parametrize("path", fixtures("rerank_"))
def test_rerank_matches_reference_fixture(vaqlib, path):
    g = np.load(path)
    X = g["X"]
    bv = VaqBitVec(0, int(g["n_bits"]))
    bv.set_rows(g["rows"])
    for as_bytes in (True, False):
        r = VaqRefiner(X.shape[1], 0)
        if as_bytes:
            r.set_rows_u8(X)
        else:
            r.set_rows(X.astype(np.float32))
        lab, dis = bv.query_rerank(g["queries"], g["XQ"], int(g["k"]), int(g["factor"]), r)
        assert np.array_equal(lab, g["labels"])
        assert np.array_equal(dis, g["dists"])
        r.close()
    bv.close()


# (n_bits, n, nq, k): every W of {1, 2, 3, 5, 16}; n around 32, around k, one row tile + 1, several workgroups;
# nq = 1, query tile - 1, query tile + 1; k = 1, 17, 100, 1024
SHAPES = [
    (64, 1, 1, 1), (64, 31, 63, 17), (128, 32, 65, 17), (150, 33, 1, 100), (300, 99, 3, 100), (320, 100, 3, 100),
    (100, 101, 3, 100), (1000, 513, 2, 17), (1024, 5000, 65, 100), (150, 5000, 63, 1), (64, 1023, 2, 1024),
    (128, 1024, 1, 1024), (257, 1025, 2, 1024),
]


@pytest.mark.parametrize("n_bits,n,nq,k", SHAPES)
def test_query_against_restatement(vaqlib, n_bits, n, nq, k):
    rs = np.random.RandomState(n_bits * 7 + n)
    W = (n_bits + 63) // 64
    rows = words(rs, n, W)
    if n >= 1000:  # half the rows near the first query: its k best are a crowd of small, equal distances
        rows[::2] = near(rs, rows[0], (n + 1) // 2, 6)
    queries = words(rs, nq, W)
    queries[0] = rows[0]
    if n_bits % 64:
        tail = np.uint64((1 << (64 - n_bits % 64)) - 1)
        assert (rows[:, -1] & tail).any() and (queries[:, -1] & tail).any()
    bv = VaqBitVec(0, n_bits)
    bv.set_rows(rows, id_base=1000)
    assert len(bv) == n
    want_l, want_d = br.query_sort(rows, queries, k, id_base=1000)
    lab, dis = bv.query(queries, k)
    assert np.array_equal(lab, want_l)
    assert np.array_equal(dis, want_d)
    bv.close()


def test_add_rows_and_all_equal_rows(vaqlib):
    rs = np.random.RandomState(3)
    row = words(rs, 1, 2)
    rows = np.repeat(row, 700, axis=0)  # every distance ties
    queries = words(rs, 3, 2)
    bv = VaqBitVec(0, 128)
    bv.set_rows(rows[:40], id_base=7)
    bv.add_rows(rows[40:41])
    bv.add_rows(rows[41:])
    assert len(bv) == 700
    for k in (17, 100):
        want = br.query_sort(rows, queries, k, id_base=7)
        got = bv.query(queries, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # appended rows that differ, behind a set that replaced everything
    more = words(rs, 50, 2)
    bv.set_rows(rows[:10])
    bv.add_rows(more)
    want = br.query_sort(np.concatenate([rows[:10], more]), queries, 17)
    got = bv.query(queries, 17)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    bv.close()


def test_two_chunks_give_the_same_answer(vaqlib):
    rs = np.random.RandomState(4)
    rows, queries = words(rs, 100, 3), words(rs, 5, 3)
    bv = VaqBitVec(0, 192)
    bv.set_rows(rows)
    want = br.query_sort(rows, queries, 17)
    bv.set_option("dist_chunk_bytes", 3 * 128 * 2)  # three queries of 128 padded rows: chunks of 3 and 2
    got = bv.query(queries, 17)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(VaqHipError) as e:
        bv.set_option("dist_chunk_bytes", 0)
    assert e.value.code == -1
    with pytest.raises(VaqHipError) as e:
        bv.set_option("no_such_option", 1)
    assert e.value.code == -1
    bv.close()


def test_device_form_on_another_stream(vaqlib):
    import torch
    rs = np.random.RandomState(6)
    rows, queries = words(rs, 600, 2), words(rs, 9, 2)
    X = rs.randint(0, 256, (600, 8)).astype(np.uint8)
    XQ = rs.randint(0, 256, (9, 8)).astype(np.float32)
    bv = VaqBitVec(0, 128)
    bv.set_rows(torch.from_numpy(rows.view(np.int64)).cuda())
    r = VaqRefiner(8, 0)
    r.set_rows_u8(X)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(queries.view(np.int64)).cuda()
        doq = torch.from_numpy(XQ).cuda()
        lab, dis = bv.query_device(dq, 20)
        rl, rd = bv.query_rerank_device(dq, doq, 10, 4, r)
    s.synchronize()
    want_l, want_d = br.query_sort(rows, queries, 20)
    assert np.array_equal(lab.cpu().numpy(), want_l)
    assert np.array_equal(dis.cpu().numpy(), want_d.astype(np.float32))
    want_l, want_d = br.query_rerank(rows, queries, X, XQ, 10, 4)
    assert np.array_equal(rl.cpu().numpy(), want_l)
    assert np.array_equal(rd.cpu().numpy(), want_d)
    r.close()
    bv.close()


# (D, n, k, factor): factor 1, 2, 10; factor * k > n (the clamp, also below k); factor * k = 1024
RERANK = [(1, 200, 10, 1), (7, 200, 17, 2), (128, 400, 10, 10), (7, 30, 17, 2), (16, 12, 17, 3), (128, 1100, 512, 2),
          (16, 1100, 128, 8)]


@pytest.mark.parametrize("D,n,k,factor", RERANK)
def test_rerank_against_restatement(vaqlib, D, n, k, factor):
    rs = np.random.RandomState(D * 31 + n + k)
    rows = near(rs, words(rs, 1, 2)[0], n, 9)
    queries = near(rs, rows[0], 3, 5)
    # byte rows: integer distances, equal ones everywhere (a narrow range where D is large)
    Xb = rs.randint(0, 256 if D < 16 else 3, (n, D)).astype(np.uint8)
    XQb = rs.randint(0, 256 if D < 16 else 3, (3, D)).astype(np.float32)
    bv = VaqBitVec(0, 128)
    bv.set_rows(rows, id_base=50)
    want = br.query_rerank(rows, queries, Xb, XQb, k, factor, id_base=50)
    for as_bytes in (True, False):
        r = VaqRefiner(D, 0)
        if as_bytes:
            r.set_rows_u8(Xb, id_base=50)
        else:
            r.set_rows(Xb.astype(np.float32), id_base=50)
        lab, dis = bv.query_rerank(queries, XQb, k, factor, r)
        assert np.array_equal(lab, want[0])
        assert np.array_equal(dis, want[1])
        r.close()
    # general float data: the distance is the reference's own loop, float32 step by step
    Xf = rs.standard_normal((n, D)).astype(np.float32) * np.float32(37.5)
    XQf = rs.standard_normal((3, D)).astype(np.float32) * np.float32(37.5)
    r = VaqRefiner(D, 0)
    r.set_rows(Xf, id_base=50)
    want = br.query_rerank(rows, queries, Xf, XQf, k, factor, id_base=50)
    lab, dis = bv.query_rerank(queries, XQf, k, factor, r)
    assert np.array_equal(lab, want[0])
    assert np.array_equal(dis, want[1])
    r.close()
    bv.close()


def test_refusals(vaqlib):
    """every refusal is a host-side return: nothing here reaches a kernel"""
    rs = np.random.RandomState(8)
    rows, queries = words(rs, 300, 1), words(rs, 2, 1)
    X = rs.randint(0, 9, (300, 4)).astype(np.uint8)
    XQ = np.zeros((2, 4), np.float32)
    with pytest.raises(VaqHipError) as e:
        VaqBitVec(0, 1025)
    assert e.value.code == -2
    with pytest.raises(VaqHipError) as e:
        VaqBitVec(0, 0)
    assert e.value.code == -1
    bv = VaqBitVec(0, 64)
    assert bv.query(queries, 3)[0].tolist() == [[-1] * 3] * 2  # no rows yet: every slot empty
    bv.set_rows(rows)
    r = VaqRefiner(4, 0)
    r.set_rows_u8(X)

    def code(fn):
        with pytest.raises(VaqHipError) as e:
            fn()
        return e.value.code, str(e.value)

    assert code(lambda: bv.query(queries, 0))[0] == -1
    assert code(lambda: bv.query(queries, 1025))[0] == -2
    for m in (QueryMethod.Heap, QueryMethod.HeapEarlyAbandon, QueryMethod.SortEarlyAbandon):
        c, text = code(lambda: bv.query(queries, 3, m))
        assert c == -2 and "equal" in text and "Sort" in text
    assert code(lambda: bv.query(queries, 3, 7))[0] == -1
    assert code(lambda: bv.query(queries.astype(np.int64), 3))[0] == -1
    assert code(lambda: bv.query_rerank(queries, XQ, 3, 0, r))[0] == -1
    assert code(lambda: bv.query_rerank(queries, XQ, 205, 5, r))[0] == -2  # 1025 candidates
    assert code(lambda: bv.query_rerank(queries, XQ, 1025, 1, r))[0] == -2
    lab, _ = bv.query_rerank(queries, XQ, 256, 4, r)  # 1024 candidates, clamped to the 300 rows
    assert (lab[:, :256] >= 0).all()
    # a refiner that does not describe the engine's rows
    r.set_rows_u8(X[:299])
    assert code(lambda: bv.query_rerank(queries, XQ, 3, 2, r))[0] == -7
    r.set_rows_u8(X, id_base=1)
    assert code(lambda: bv.query_rerank(queries, XQ, 3, 2, r))[0] == -7
    # nq == 0 succeeds
    lab, dis = bv.query(np.zeros((0, 1), np.uint64), 5)
    assert lab.shape == (0, 5) and dis.shape == (0, 5)
    r.set_rows_u8(X)
    lab, dis = bv.query_rerank(np.zeros((0, 1), np.uint64), np.zeros((0, 4), np.float32), 5, 2, r)
    assert lab.shape == (0, 5)
    r.close()
    bv.close()


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/bitvec_shim_test.cpp: BitVecEngineHip::loadBitV / loadOriginal / query / queryRerank of
    include/vaqhip.hpp against the answers of the restatement, written to argv[1]"""
    import subprocess
    from vaq_amd import build
    rs = np.random.RandomState(12)
    n, nq, W, D, k, factor = 400, 5, 2, 8, 10, 3
    rows = near(rs, words(rs, 1, W)[0], n, 8)
    queries = near(rs, rows[0], nq, 4)
    X = rs.randint(0, 6, (n, D)).astype(np.uint8)
    XQ = rs.randint(0, 6, (nq, D)).astype(np.float32)
    ql, qd = br.query_sort(rows, queries, k)
    rl, rd = br.query_rerank(rows, queries, X, XQ, k, factor)
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([n, nq, W, D, k, factor], np.int32).tobytes())
        for a in (rows, queries, X, XQ, ql, qd, rl, rd):
            f.write(np.ascontiguousarray(a).tobytes())
    lib = build.build_lib()
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "bitvec_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "bitvec_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bitvec_shim ok" in out.stdout, out.stdout + out.stderr
