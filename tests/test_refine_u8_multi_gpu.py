"""Byte rows across the shards of a multi-device refiner (vaqhip_multi_refiner_*_u8): refine, the exhaustive form and
the fused call answer as the single byte refiner does (itself equal to the float refiner: test_refine_u8_gpu.py), and
the encode across the shards reads byte rows through the widen kernel and gives the codes of the widened host matrix.
Logical shards on device 0 ([0, 0, 0], and [0]: the single refiner's launches) exercise every path on one GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

from helpers import make_case

pytestmark = pytest.mark.gpu

DEVICES = [[0, 0, 0], [0]]
IDS = ["g3", "g1"]
ESTATE = -7


def equal(a, b):
    return np.array_equal(a.labels, b.labels) and np.array_equal(np.asarray(a.distances, np.float32).view(np.uint32),
                                                                 np.asarray(b.distances, np.float32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def rows(D=32, N=1000):
    """byte rows with 0 and 255 in every row, a fifth of them copies of other rows; 9 queries, two of them byte-valued"""
    rng = np.random.default_rng(D + N)
    X = rng.integers(0, 256, size=(N, D), dtype=np.uint8)
    col = (np.arange(N) * 5 + 1) % D
    X[np.arange(N), col] = 255
    X[np.arange(N), (col + 1) % D] = 0
    X[rng.integers(0, N, N // 5)] = X[rng.integers(0, N, N // 5)]
    Xq = rng.uniform(0, 255, size=(9, D)).astype(np.float32)
    Xq[0], Xq[5] = X[N // 2], rng.integers(0, 256, D)
    return np.ascontiguousarray(X), Xq


def check_refine_and_search(m, one, Xq, N, id_base, what):
    rng = np.random.default_rng(N)
    R = min(N + 3, 200)
    cand = (id_base + np.stack([rng.permutation(N + 3)[:R] - 1 for _ in range(len(Xq))])).astype(np.int32)
    for exact in (False, True):
        m.exact_ties = one.exact_ties = exact
        for k in (1, min(10, R)):
            assert equal(m.refine(Xq, cand, k), one.refine(Xq, cand, k)), (what, "refine", exact, k)
        for k in (1, 10, N + 5):
            assert equal(m.search(Xq, k), one.search(Xq, k)), (what, "search", exact, k)


@pytest.mark.parametrize("devices", DEVICES, ids=IDS)
def test_refine_and_search(vaqlib, devices):
    """N = 1000 (not divisible by 3), N = 2 (an empty shard), and add_rows_u8 onto the last shard"""
    import vaq_amd
    X, Xq = rows()
    D = X.shape[1]
    m, one = vaq_amd.VaqMultiRefiner(devices, D), vaq_amd.VaqRefiner(D)
    assert m.elem_size == 4
    for N in (1000, 2):
        m.set_rows_u8(X[:N], id_base=40)
        one.set_rows_u8(X[:N], id_base=40)
        assert m.elem_size == 1 and m.info()["N"] == N
        if len(devices) == 3:
            assert m.info()["shard_rows"] == ([334, 334, 332] if N == 1000 else [1, 1, 0])
        check_refine_and_search(m, one, Xq, N, 40, (devices, N))
    m.add_rows_u8(X[2:700])
    one.add_rows_u8(X[2:700])
    if len(devices) == 3:
        assert m.info()["shard_rows"] == [1, 1, 698]
    check_refine_and_search(m, one, Xq, 700, 40, (devices, "appended"))
    with pytest.raises(vaq_amd.VaqHipError) as e:
        m.add_rows(X[:3].astype(np.float32))
    assert e.value.code == ESTATE and m.elem_size == 1
    m.set_rows(X[:50].astype(np.float32))
    assert m.elem_size == 4
    with pytest.raises(vaq_amd.VaqHipError) as e:
        m.add_rows_u8(X[:3])
    assert e.value.code == ESTATE
    m.set_rows_u8(X[:0])
    m.add_rows_u8(X[:300])  # a refiner without rows takes either type: the last shard takes them
    one.set_rows_u8(X[:300])
    assert m.elem_size == 1
    check_refine_and_search(m, one, Xq, 300, 0, (devices, "from empty"))
    m.close(), one.close()


@functools.lru_cache(maxsize=None)
def index_case():
    """a byte-code index over 1000 rows of 32 dims and the byte rows its candidates are refined against"""
    c = make_case(977, 32, [8] * 8, 1000, 9, dup_frac=0.2, rotate=False, scale=60.0)
    X, _ = rows()
    c["X"] = (c["X"] + 128).astype(np.float32)
    return c, X


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("devices", DEVICES, ids=IDS)
def test_fused_search_refine(vaqlib, devices, exact):
    """VaqHipMulti.search_refine over byte rows == VaqHip.search_refine with the single byte refiner"""
    import vaq_amd
    from vaq_amd.index import VaqHipMulti
    c, X = index_case()
    m = VaqHipMulti(devices, c["bits"], c["cents"], c["eig"])
    m.set_codes(c["codes"])
    v = vaq_amd.VaqHip()
    v.mBitsAlloc, v.mCentroidsPerSubs, v.mCodebook = c["bits"], c["cents"], c["codes"]
    for ix in (m, v):
        ix.set_option("exact_ties", 1 if exact else 0)
    mr, r = vaq_amd.VaqMultiRefiner(devices, 32), vaq_amd.VaqRefiner(32)
    mr.set_rows_u8(X)
    r.set_rows_u8(X)
    mr.exact_ties = r.exact_ties = exact
    assert equal(m.search_refine(c["X"], 100, 10, mr), v.search_refine(c["X"], 100, 10, r))
    for x in (m, v, mr, r):
        x.close()


@pytest.mark.parametrize("devices", DEVICES, ids=IDS)
def test_encode_from_byte_refiner(vaqlib, devices):
    """encode_from_refiner over a byte refiner == encode(widened host matrix), code for code, with encode_chunk_rows =
    100 at N = 1000 so that every shard widens several chunks and a short last one (334 = 3 * 100 + 34)"""
    import vaq_amd
    from vaq_amd.index import VaqHipMulti
    X, Xq = rows()
    c = make_case(978, 32, [8, 7, 6, 5], 0, 1, rotate=True, scale=60.0)
    a = VaqHipMulti(devices, c["bits"], c["cents"], c["eig"])
    b = VaqHipMulti(devices, c["bits"], c["cents"], c["eig"])
    want = b.encode(X.astype(np.float32), projected=False, id_base=7, return_codes=True)
    r = vaq_amd.VaqMultiRefiner(devices, 32)
    r.set_rows_u8(X, id_base=7)
    a.set_option("encode_chunk_rows", 100)
    got = a.encode_from_refiner(r, return_codes=True)
    assert np.array_equal(got, want)
    assert a.info()["shard_rows"] == b.info()["shard_rows"] and a.info()["id_base"] == 7
    for k in (1, 10):
        assert equal(a.search(Xq, k), b.search(Xq, k))
    for x in (a, b, r):
        x.close()


@pytest.mark.parametrize("devices", DEVICES, ids=IDS)
def test_encode_lut_from_byte_refiner(vaqlib, devices):
    """the engine's encoder over a byte refiner == encode_lut(widened host matrix), code for code"""
    import test_lutfit_multi_gpu as lm
    import vaq_amd
    X, _ = rows(8, 1000)
    Xf = X.astype(np.float32)
    bits = [8, 6, 5, 4, 3, 2, 1, 7]
    rc, cent, Qs = lm.single_fit(vaqlib, Xf, bits)
    assert rc == 0
    c = dict(bits=bits, cent=cent, Qs=Qs, eig=None)
    a, b = lm.seq_multi(c, len(devices)), lm.seq_multi(c, len(devices))
    for x in (a, b):
        x.set_lut_quantiles(Qs)
    want = b.encode_lut(Xf, projected=False, return_codes=True)
    r = vaq_amd.VaqMultiRefiner(devices, 8)
    r.set_rows_u8(X)
    a.set_option("encode_chunk_rows", 100)
    got = a.encode_lut_from_refiner(r, return_codes=True)
    assert np.array_equal(got, want)
    for x in (a, b, r):
        x.close()


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/refine_u8_shim_test.cpp: VaqHip::setRefineDataset(RowMatrix<uint8_t>), then search(XTest, k, refineNum),
    searchExhaustive and encodeRefineDataset() on one device and after setDevices({0, 0}), against the float overload"""
    from vaq_amd import build
    N, M, L, bits, nq = 3000, 8, 4, 8, 9
    c = make_case(734, M * L, [bits] * M, N, nq, dup_frac=0.2, rotate=False, scale=60.0)
    base, _ = rows(M * L, N)
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([N, M, L, bits, nq], np.int32).tobytes())
        f.write(np.ascontiguousarray(c["codes"]).tobytes())
        for cent in c["cents"]:
            f.write(np.ascontiguousarray(cent + 128, np.float32).tobytes())
        f.write(base.tobytes())
        f.write(np.ascontiguousarray(c["X"] + 128, np.float32).tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "refine_u8_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "refine_u8_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refine_u8_shim ok" in r.stdout, r.stdout + r.stderr
