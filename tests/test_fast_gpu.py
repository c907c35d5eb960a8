"""FAST search method on the GPU against the NumPy checker (tests/fast_ref.py), slot
for slot: labels and distances with np.array_equal.  The checker takes its float
tables from the existing CreateLUT hook (vaqhip_build_lut, bit-exact to the
reference: test_parity_gpu.py), so what is checked here is everything after it."""
import ctypes as C

import numpy as np
import pytest

import fast_ref as fr
from helpers import make_case

pytestmark = pytest.mark.gpu


def fast_index(c, off=None, sc=None, methods="FAST", id_base=0):
    import vaq_amd
    v = vaq_amd.VaqHipFast(device=0)
    v.parseMethodString(f"VAQ{sum(c['bits'])}m{c['M']}min1max{max(c['bits'])}var1,{methods}")
    v.mBitsAlloc = c["bits"]
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    v.id_base = id_base
    if off is not None:
        v.setLUTQuantization(off, sc)
    return v


def spread_quant(lut, frac=0.9):
    """offsets / scales that spread every column over [0, 255 * frac]"""
    lo = lut.min(axis=(0, 2)).astype(np.float32)
    hi = lut.max(axis=(0, 2)).astype(np.float32)
    sc = (np.float32(255 * frac) / np.maximum(hi - lo, np.float32(1e-3))).astype(np.float32)
    return lo, sc


def check(v, c, k, lut, projected=False, what=""):
    ans = v.search(c["X"], k, projected=projected)
    nq = c["X"].shape[0]
    el, ed = fr.search_fast(lut, v.mOffsets, v.mScale, c["codes"], k, id_base=v.id_base)
    lab = ans.labels.reshape(nq, k)
    dis = ans.distances.reshape(nq, k)
    assert np.array_equal(dis, ed), what
    assert np.array_equal(lab, el.astype(np.int32)), what
    return lab, dis


# A row packs at most 256 code bits, so 4-bit codes stop at M = 64; FAST itself serves every M up to 128
# (narrower codes: 80 x 3, 96 x 2, 128 x 2 bits and a 1/2-bit mix; searched in test_fast_shapes_gpu.py)
@pytest.mark.parametrize("bits", [[4] * 8, [4] * 16, [4] * 32, [4] * 64, [4, 4, 3, 3, 2, 2, 1, 1],
                                  [4] * 4, [4] * 12, [4] * 20, [4] * 36, [4] * 40, [3] * 80, [2] * 96, [2] * 128,
                                  [2, 1] * 64])
def test_small_lut_bytes(vaqlib, bits):
    M = len(bits)
    c = make_case(11, 2 * M if M > 8 else 16, bits, 100, 9)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    off, sc = spread_quant(lut)
    off[0] = lut.max()  # a column quantised to all zeros ...
    off[1] = -5.0       # ... one whose padding rows (zero tables) are not 0
    v.setLUTQuantization(off, sc)
    got = v.buildSmallLUT(c["X"])
    assert np.array_equal(got, fr.small_lut16(lut, off, sc))
    v.close()


CASES = [  # N, k, nq
    (1, 16, 5), (15, 16, 5), (33, 17, 20), (1000, 1, 50), (1000, 16, 40), (1000, 100, 50),
    (1000, 1024, 8), (100000, 100, 64), (100000, 1024, 16), (5000, 17, 1000),
]


@pytest.mark.parametrize("N,k,nq", CASES)
def test_search_matches_checker(vaqlib, N, k, nq):
    c = make_case(100 + N + k, 64, [4] * 16, N, nq, dup_frac=0.05)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    check(v, c, k, lut, what=f"N={N} k={k}")
    v.close()


@pytest.mark.parametrize("levels", [0, 3])
def test_massive_ties(vaqlib, levels):
    """scale so small that every table entry is 0 (all distances equal) or 0..2"""
    c = make_case(7, 32, [4] * 8, 20000, 24)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    lo, hi = lut.min(axis=(0, 2)), lut.max(axis=(0, 2))
    sc = np.full(8, 1e-9, np.float32) if levels == 0 else (levels / (hi - lo)).astype(np.float32)
    v.setLUTQuantization(lo, sc)
    for k in (16, 17, 100, 1024):
        check(v, c, k, lut, what=f"levels={levels} k={k}")
    v.close()


def test_identical_rows_id_base_and_append(vaqlib):
    c = make_case(8, 32, [4, 4, 3, 3, 2, 2, 1, 1], 3000, 30)
    c["codes"][:] = c["codes"][5]
    v = fast_index(c, id_base=1000)
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    check(v, c, 100, lut, what="identical rows")
    extra = make_case(9, 32, [4, 4, 3, 3, 2, 2, 1, 1], 2500, 1)["codes"]
    v.add_codes(extra)
    c2 = dict(c, codes=np.concatenate([c["codes"], extra]))
    check(v, c2, 100, lut, what="after add_codes")
    check(v, c2, 1024, lut, what="after add_codes, k=1024")
    v.close()


def test_device_and_projected_entry_points(vaqlib):
    import torch
    c = make_case(12, 64, [4] * 16, 40000, 70)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    el, ed = check(v, c, 50, lut, what="host")
    Xp = v.project(c["X"])
    cp = dict(c, X=Xp)
    check(v, cp, 50, lut, projected=True, what="host projected")
    q = torch.from_numpy(c["X"]).cuda()
    lab, dis = v.search_device(q, 50)
    torch.cuda.synchronize()
    assert np.array_equal(lab.cpu().numpy(), el) and np.array_equal(dis.cpu().numpy(), ed)
    lab, dis = v.search_device(torch.from_numpy(Xp).cuda(), 50, projected=True)
    torch.cuda.synchronize()
    assert np.array_equal(lab.cpu().numpy(), el) and np.array_equal(dis.cpu().numpy(), ed)
    v.close()


def test_one_million_encoded_rows(vaqlib):
    rng = np.random.default_rng(5)
    D, M, N = 128, 64, 1 << 20
    c = make_case(13, D, [4] * M, 1, 32)
    data = (rng.normal(size=(N, D)) * 30).astype(np.float32)
    v = fast_index(c)
    v.encode(data, projected=False)
    assert v.mCodebookCMajor.shape == (N, M) and np.isfortran(v.mCodebookCMajor)
    c["codes"] = v.mCodebook
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    check(v, c, 100, lut, what="1M rows")
    v.close()


def test_learn_quantization(vaqlib):
    c = make_case(14, 64, [4] * 16, 30000, 40)
    rng = np.random.default_rng(3)
    train = (rng.normal(size=(20000, 64)) * 30).astype(np.float32)
    v = fast_index(c)
    v.learnQuantization(train, 0.05)
    rows = fr.sample_rows(train.shape[0], 0.05)
    assert rows.shape[0] == 1000
    luts = fr.stack_luts(v.build_lut(train[rows]))
    off, sc, _ = fr.learn_from_luts(luts)
    assert np.array_equal(v.mOffsets, off) and np.array_equal(v.mScale, sc)
    lut = v.build_lut(c["X"])
    check(v, c, 100, lut, what="learned quantisation")
    v.close()


def test_fast_heap_is_heap(vaqlib):
    c = make_case(15, 64, [4] * 16, 20000, 20)
    v = fast_index(c, methods="HEAP_FAST")
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    a = v.search(c["X"], 30)
    h = fast_index(c, methods="HEAP")
    b = h.search(c["X"], 30)
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.distances, b.distances)
    v.close()
    h.close()


def test_error_codes(vaqlib):
    import vaq_amd
    from vaq_amd import _lib
    L = _lib.load()
    c = make_case(16, 32, [4] * 8, 500, 4)
    v = fast_index(c)
    v._ensure_codes()
    h = v._h
    X = c["X"]
    lab = np.empty((4, 10), np.int32)
    dis = np.empty((4, 10), np.float32)

    def search(k=10):
        return L.vaqhip_search(h, X.ctypes.data_as(C.c_void_p), 4, k, lab.ctypes.data_as(C.c_void_p),
                               dis.ctypes.data_as(C.c_void_p))
    assert L.vaqhip_index_set_method(h, 0x08, C.c_float(1.0)) == 0
    assert search() == -7 and b"quantization" in L.vaqhip_last_error()  # no quantisation yet
    small = np.empty((4, 8, 16), np.uint8)
    assert L.vaqhip_build_small_lut(h, X.ctypes.data_as(C.c_void_p), 4, 0, small.ctypes.data_as(C.c_void_p)) == -7
    one, zero = np.ones(8, np.float32), np.zeros(8, np.float32)
    nan = np.full(8, np.nan, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.vaqhip_index_set_lut_quantization(h, p(zero), p(zero)) == -1
    assert L.vaqhip_index_set_lut_quantization(h, p(nan), p(one)) == -1
    assert L.vaqhip_index_set_lut_quantization(h, p(zero), p(-one)) == -1
    assert L.vaqhip_index_set_lut_quantization(h, p(zero), p(one)) == 0
    assert search() == 0
    assert search(1025) == -2
    assert L.vaqhip_index_set_method(h, 0x01, C.c_float(1.0)) == -2   # SORT
    assert L.vaqhip_index_set_method(h, 0x18, C.c_float(1.0)) == -2   # FAST2
    assert L.vaqhip_search_staged_supported(h, 16, 10) == 0
    thr = np.empty(4, np.int32)
    assert L.vaqhip_search_begin_device(h, None, 4, 10, 0, None, None, p(thr), None) == -2
    tr = np.empty((4, 2 * c["L"]), np.float32)
    train = np.zeros((9, 32), np.float32)
    assert L.vaqhip_learn_quantization(h, p(train), 9, 0, C.c_float(0.1), None, None) == -1
    # FAST alone on a TI-grouped index is a state error at search
    tr[:] = np.random.default_rng(0).normal(size=tr.shape)
    assert L.vaqhip_index_set_ti_clusters(h, p(tr), 4, 2) == 0
    assert L.vaqhip_index_set_method(h, 0x08, C.c_float(1.0)) == 0
    assert search() == -7
    v.close()
    # wider codes, the sequential sum, and the multi-device index refuse FAST
    w = make_case(17, 32, [8] * 8, 10, 1)
    hv = vaq_amd.VaqHip(device=0)
    hv.mBitsAlloc, hv.mCentroidsPerSubs, hv.mEigenVectors, hv.mCodebook = w["bits"], w["cents"], None, w["codes"]
    hv._ensure_codes()
    assert L.vaqhip_index_set_method(hv._h, 0x08, C.c_float(1.0)) == -2
    assert L.vaqhip_index_set_lut_quantization(hv._h, p(zero), p(one)) == -2
    hv.close()
    s = vaq_amd.VaqHip(device=0, sequential_sum=True)
    s.mBitsAlloc, s.mCentroidsPerSubs = [4] * 6, [np.zeros((16, 1), np.float32)] * 6
    s.mCodebook = np.zeros((10, 6), np.uint16)
    s._ensure_codes()
    assert L.vaqhip_index_set_method(s._h, 0x08, C.c_float(1.0)) == -2
    s.close()
    mx = vaq_amd.index.VaqHipMulti([0, 0], c["bits"], c["cents"], None)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        mx.set_method(0x08)
    assert e.value.code == -2
    mx.close()


def test_queries_past_the_first_chunk(vaqlib):
    """4M rows: a chunk of the FAST search holds 2^29 / 4M = 128 queries, so 130 queries take two;
    queries on both sides of the cut are checked"""
    c = make_case(18, 32, [4] * 8, 1 << 22, 130, rotate=False)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    k = 20
    ans = v.search(c["X"], k)
    lab = ans.labels.reshape(130, k)
    dis = ans.distances.reshape(130, k)
    for q in (0, 1, 127, 128, 129):
        el, ed = fr.search_fast(lut[q:q + 1], v.mOffsets, v.mScale, c["codes"], k)
        assert np.array_equal(dis[q], ed[0]) and np.array_equal(lab[q], el[0].astype(np.int32)), q
    v.close()


def test_code_image_follows_the_method(vaqlib):
    """the FAST code image is built at the first FAST search, dropped when another method is set and
    rebuilt from the packed codes (also after appends made while FAST was not in force)"""
    from vaq_amd import NNMethod
    c = make_case(19, 32, [4, 4, 3, 3, 2, 2, 1, 1], 6000, 12)
    v = fast_index(c, methods="HEAP")
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    v.search(c["X"], 10)
    extra = make_case(20, 32, [4, 4, 3, 3, 2, 2, 1, 1], 3000, 1)["codes"]
    v.add_codes(extra)                       # appended while HEAP is in force: no image
    c2 = dict(c, codes=np.concatenate([c["codes"], extra]))
    v.mMethods = NNMethod.Fast
    check(v, c2, 100, lut, what="image built at the first FAST search")
    more = make_case(21, 32, [4, 4, 3, 3, 2, 2, 1, 1], 2000, 1)["codes"]
    v.add_codes(more)                        # appended while FAST is in force: the image grows
    c3 = dict(c2, codes=np.concatenate([c2["codes"], more]))
    check(v, c3, 100, lut, what="image extended by an append")
    v.mMethods = NNMethod.Heap
    v.search(c["X"], 10)                     # image released
    v.mMethods = NNMethod.Fast
    check(v, c3, 17, lut, what="image rebuilt")
    v.mCodebook = c["codes"].copy()          # codes replaced while FAST is in force
    check(v, c, 100, lut, what="codes replaced")
    v.close()


def test_demo_driver_fast(vaqlib, tmp_path):
    """examples/demo_vaqhip.cpp with a FAST method string and --learn-ratio (demo_vaq.cpp:120-124)
    returns what VaqHipFast returns after learnQuantization on the same dataset"""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    c = make_case(22, 64, [4] * 16, 20000, 15)
    rng = np.random.default_rng(4)
    dataset = (rng.normal(size=(8000, 64)) * 30).astype(np.float32)
    io.save_centroids(c["cents"], str(tmp_path / "c.bin"))
    io.save_codebook(c["codes"], str(tmp_path / "cb.bin"))
    c["eig"].astype(np.float32).tofile(str(tmp_path / "e.f32"))
    io.write_vecs(str(tmp_path / "q.fvecs"), c["X"])
    io.write_vecs(str(tmp_path / "base.fvecs"), dataset)
    r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                        "--eigen", str(tmp_path / "e.f32"), "--queries", str(tmp_path / "q.fvecs"),
                        "--timeseries-size", "64", "--k", "100", "--method", "VAQ64m16min4max4var1,FAST",
                        "--dataset", str(tmp_path / "base.fvecs"), "--learn-ratio", "0.1",
                        "--result", str(tmp_path / "out.csv")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Learn Quantization time" in r.stdout
    got = np.loadtxt(str(tmp_path / "out.csv"), delimiter=",", dtype=np.int64)
    v = fast_index(c)
    v.learnQuantization(dataset, 0.1)
    ans = v.search(c["X"], 100)
    assert np.array_equal(got, ans.labels.reshape(15, 100).astype(np.int64))
    lut = v.build_lut(c["X"])
    check(v, c, 100, lut, what="demo's quantisation")
    v.close()
    # the same string with 8-bit codes is refused, as the reference refuses it
    r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                        "--queries", str(tmp_path / "q.fvecs"), "--timeseries-size", "64",
                        "--method", "VAQ128m16min8max8var1,FAST", "--dataset", str(tmp_path / "base.fvecs")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "> 4" in r.stderr
