"""Building an index from byte rows on the GPU: the *_u8 forms of encode, encode_lut and the quantile fits (single and
sharded), the byte refiner in the sharded fit, and the adapters above them.

(float)uint8 is exact and a byte is widened where a kernel loads it, so every expected value here is the FLOAT form of
the same call on X.astype(float32), compared with array_equal (fit outputs as bit patterns).  There is no tolerance
anywhere.  Every matrix of byte rows holds 0, 255 and values >= 128 (a signed load would show at once).  Logical shards
of device 0 ([0] * G) exercise every sharded path on one GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import lutfit_ref as lr
import seq_exact_ref as sr
from helpers import make_case

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
EINVAL = -1


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    bad = np.argwhere(u32(got) != u32(want))
    assert bad.size == 0, f"{what}: {len(bad)} differ, first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


@functools.lru_cache(maxsize=None)
def byte_rows(n, D, seed=0):
    """n x D bytes over the whole range; row 0 starts 0, 255, 128 (as far as D allows), and every row of a matrix with
    D >= 3 holds a 255, a 0 and a 128 somewhere"""
    rng = np.random.default_rng(1000 * D + n + seed)
    X = rng.integers(0, 256, size=(n, D), dtype=np.uint8)
    if D >= 3:
        col = (np.arange(n) * 5 + 1) % D
        X[np.arange(n), col] = 255
        X[np.arange(n), (col + 1) % D] = 0
        X[np.arange(n), (col + 2) % D] = 128
    flat = X.reshape(-1)
    flat[:min(3, flat.size)] = np.array([0, 255, 128], np.uint8)[:min(3, flat.size)]
    X = np.ascontiguousarray(X)
    X.setflags(write=False)
    return X


def holds_the_edges(X):
    return bool((X == 0).any() and (X == 255).any() and (X >= 128).any())


def rotation(D, seed=0):
    rng = np.random.default_rng(77 + D + seed)
    return np.ascontiguousarray(np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32))


# ---- projection + encode, one index ----
# (D, n, bits): the tile kernel with 8 rows per thread (2048 <= n < 65536) and 16 (n >= 65536), each with a short last
# tile; the row-per-workgroup kernel below 2048 rows and at every D the tile kernel does not take
ENCODE_SHAPES = [(64, 2048 + 3, [8, 7, 6, 5]), (128, 65536 + 5, [8] * 8), (256, 65536 + 1, [8] * 8), (128, 2047, [8] * 8),
                 (20, 300, [8, 7, 6, 5]), (100, 300, [8] * 4), (300, 200, [8, 7, 6, 5])]


@pytest.mark.parametrize("D,n,bits", ENCODE_SHAPES, ids=[f"D{d}_n{n}" for d, n, _ in ENCODE_SHAPES])
def test_encode_one_index(vaqlib, D, n, bits):
    """encode_u8 == encode on the widened rows, code for code: projected=False with a rotation (the byte projection) and
    projected=True (no projection: the chunk is widened on the device)"""
    import vaq_amd
    X = byte_rows(n, D)
    assert holds_the_edges(X)
    Xf = X.astype(np.float32)
    c = make_case(D, D, bits, 0, 1, rotate=True, scale=60.0)
    v = vaq_amd.VaqHip()
    v.mBitsAlloc, v.mCentroidsPerSubs, v.mEigenVectors = c["bits"], [cc + 100 for cc in c["cents"]], c["eig"]
    for projected in (False, True):
        v.encode(Xf, projected=projected)
        want = np.array(v.mCodebook)
        v.encode_u8(X, projected=projected)
        assert np.array_equal(v.mCodebook, want), (D, n, projected)
        assert len(np.unique(want)) > 8  # (the codes are not one value: the comparison shows something)
    v.close()


def test_encode_sequential_index_without_rotation(vaqlib):
    """a VAQHIP_SUM_SEQUENTIAL index projects with checking even without eigenvectors: project_kernel's identity path
    over byte rows; and encodeLUT_u8 without a rotation widens the chunk"""
    import vaq_amd
    D, n = 20, 700
    X = byte_rows(n, D)
    Xf = X.astype(np.float32)
    bits = [int(b) for b in np.random.default_rng(4).integers(1, 9, size=D)]
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = bits
    v.fitQuantiles(Xf)
    cent, q = v.centroidsMat.copy(), v.mQuantiles.copy()
    v.fitQuantiles_u8(X)
    same_bits(v.centroidsMat, cent, "fitQuantiles_u8 centres")
    same_bits(v.mQuantiles, q, "fitQuantiles_u8 quantiles")
    for projected in (False, True):
        v.encode(Xf, projected=projected)
        want = np.array(v.mCodebook)
        v.encode_u8(X, projected=projected)
        assert np.array_equal(v.mCodebook, want)
        v.encodeLUT(Xf, projected=projected)
        want = np.array(v.mCodebook)
        v.encodeLUT_u8(X, projected=projected)
        assert np.array_equal(v.mCodebook, want)
    v.close()


def test_device_forms_at_every_byte_offset(vaqlib):
    """encode_u8_device and encodeLUT_u8_device on a torch uint8 view that starts at byte 0, 1, 2 and 3 of one
    allocation: all four equal the host form (packed loads only where the address is 4-byte aligned)"""
    import torch
    import vaq_amd
    D, n = 128, 4096 + 7
    X = byte_rows(n, D)
    Xf = X.astype(np.float32)
    c = make_case(5, D, [8, 7, 6, 5] * 2, 0, 1, rotate=True, scale=60.0)
    v = vaq_amd.VaqHip()
    v.mBitsAlloc, v.mCentroidsPerSubs, v.mEigenVectors = c["bits"], [cc + 100 for cc in c["cents"]], c["eig"]
    s = vaq_amd.VaqHip(sequential_sum=True)
    s.mBitsAlloc = [int(b) for b in np.random.default_rng(6).integers(1, 3, size=D)]  # (a row packs at most 256 bits)
    s.mEigenVectors = c["eig"]
    s.fitQuantiles_u8(X, projected=False)
    buf = torch.zeros(n * D + 3, dtype=torch.uint8, device="cuda:0")
    host = torch.from_numpy(np.array(X)).reshape(-1)
    for projected in (False, True):
        v.encode(Xf, projected=projected)
        want = np.array(v.mCodebook)
        v.encode_u8(X, projected=projected)
        assert np.array_equal(v.mCodebook, want)
        s.encodeLUT(Xf, projected=projected)
        want_lut = np.array(s.mCodebook)
        s.encodeLUT_u8(X, projected=projected)
        assert np.array_equal(s.mCodebook, want_lut)
        for off in (0, 1, 2, 3):
            view = buf[off:off + n * D]
            view.copy_(host)
            view = view.view(n, D)
            assert view.data_ptr() % 4 == off
            got = v.encode_u8_device(view, projected=projected).cpu().numpy().view(np.uint16)
            assert np.array_equal(got, want), ("encode_u8_device", off, projected)
            got = s.encodeLUT_u8_device(view, projected=projected).cpu().numpy().view(np.uint16)
            assert np.array_equal(got, want_lut), ("encodeLUT_u8_device", off, projected)
    v.close(), s.close()


# ---- the single fit ----
def fit_call(fn, X, bits, eig, *head):
    D = X.shape[1]
    cent = np.full((D, 256), SENTINEL, np.float32)
    q = np.full((D, 257), SENTINEL, np.float32)
    rc = fn(*head, _p(X), X.shape[0], D, (C.c_int * D)(*bits), _p(eig), _p(cent), _p(q))
    return rc, np.ascontiguousarray(cent.T), q


def fit_bits(D):
    return [8, 3, 1, 2, 4] if D == 5 else [int(b) for b in np.random.default_rng(D).integers(1, 9, size=D)]


@functools.lru_cache(maxsize=None)
def float_fit(n, D, with_eig):
    """vaqhip_lut_fit_quantiles on the widened rows: the yardstick of every fit below, computed once"""
    from vaq_amd import _lib
    L = _lib.load()
    rc, cent, q = fit_call(L.vaqhip_lut_fit_quantiles, byte_rows(n, D).astype(np.float32), fit_bits(D),
                           rotation(D) if with_eig else None, 0)
    assert rc == 0, L.vaqhip_last_error()
    cent.setflags(write=False), q.setflags(write=False)
    return cent, q


@pytest.mark.parametrize("with_eig", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("D,n", [(5, 1), (5, 255), (5, 1000), (40, 3000)])
def test_single_fit(vaqlib, D, n, with_eig):
    X = byte_rows(n, D)
    assert n == 1 or holds_the_edges(X)
    want_c, want_q = float_fit(n, D, with_eig)
    rc, cent, q = fit_call(vaqlib.vaqhip_lut_fit_quantiles_u8, X, fit_bits(D), rotation(D) if with_eig else None, 0)
    assert rc == 0, vaqlib.vaqhip_last_error()
    same_bits(q, want_q, "quantiles")
    same_bits(cent, want_c, "centres")
    if (D, n, with_eig) == (5, 1000, False):  # and the numpy restatement of centroidsQuantile
        ref_c, ref_q = lr.fit(X.astype(np.float32), fit_bits(D))
        same_bits(q, ref_q, "quantiles against the restatement")
        same_bits(cent, ref_c, "centres against the restatement")


# ---- the sharded fit ----
def round_widths(D, G):
    return {min(G, D - t) for t in range(0, D, G)}


def sharded_host(vaqlib, devs, X, bits, eig):
    return fit_call(vaqlib.vaqhip_multi_lut_fit_quantiles_u8, X, bits, eig, len(devs), (C.c_int * len(devs))(*devs))


def check_sharded(vaqlib, D, n, G, with_eig, forms=("host", "refiner")):
    import vaq_amd
    X, bits, eig = byte_rows(n, D), fit_bits(D), rotation(D) if with_eig else None
    want_c, want_q = float_fit(n, D, with_eig)
    devs = [0] * G
    if "host" in forms:
        rc, cent, q = sharded_host(vaqlib, devs, X, bits, eig)
        assert rc == 0, (D, n, G, vaqlib.vaqhip_multi_last_error())
        same_bits(q, want_q, f"host form D={D} n={n} G={G} eig={with_eig} quantiles")
        same_bits(cent, want_c, f"host form D={D} n={n} G={G} eig={with_eig} centres")
    if "refiner" in forms:
        r = vaq_amd.VaqMultiRefiner(devs, D)
        r.set_rows_u8(X)
        assert r.elem_size == 1
        cent, q = r.fit_quantiles(bits, eig)
        r.close()
        same_bits(q, want_q, f"byte refiner D={D} n={n} G={G} eig={with_eig} quantiles")
        same_bits(np.ascontiguousarray(cent.T), want_c, f"byte refiner D={D} n={n} G={G} eig={with_eig} centres")


@pytest.mark.parametrize("with_eig", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("D", [5, 33, 40])
def test_sharded_fit(vaqlib, D, with_eig):
    """host form and byte refiner over [0], [0, 0], [0, 0, 0] and eight logical shards; n = 7 leaves empty shards at
    G = 8, 255 / 257 straddle the column kernel's 256 rows; D = 5 and 33 end in a round narrower than G and D = 33 is
    no multiple of the 32-wide tile"""
    for n in (7, 255, 257, 1000):
        assert holds_the_edges(byte_rows(n, D))
        for G in (1, 2, 3, 8):
            check_sharded(vaqlib, D, n, G, with_eig)


WIDTH_SWEEP = (4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16)


def test_every_column_width_is_reached():
    """the rounds of test_sharded_fit and test_sharded_fit_widths together launch the column kernel with every W in
    1..16 (G = 16 at D = 40: two rounds of 16, one of 8)"""
    seen = set()
    for D in (5, 33, 40):
        for G in (1, 2, 3, 8):
            seen |= round_widths(D, G)
    for G in WIDTH_SWEEP:
        seen |= round_widths(40, G)
    assert seen == set(range(1, 17))
    assert 16 in round_widths(40, 16) and 8 in round_widths(40, 8)


@pytest.mark.parametrize("G", WIDTH_SWEEP)
def test_sharded_fit_widths(vaqlib, G):
    """D = 40 over G logical shards: W = G in the full rounds; the fused projection from the host form, the
    transposing extract from the byte refiner"""
    check_sharded(vaqlib, 40, 257, G, True, forms=("host",))
    check_sharded(vaqlib, 40, 257, G, False, forms=("refiner",))


def test_sharded_fit_refuses_infinite_eigenvectors(vaqlib):
    """an inf in the eigenvectors makes projected values infinite or NaN: EINVAL and the outputs unwritten, from the
    host form and from the byte refiner, as the float form; the next fit is sound"""
    import vaq_amd
    D, n = 5, 1000
    X, bits = byte_rows(n, D), fit_bits(D)
    eig = rotation(D).copy()
    eig[2, 3] = np.inf
    rc, cent, q = sharded_host(vaqlib, [0] * 3, X, bits, eig)
    assert rc == EINVAL and b"after the projection" in vaqlib.vaqhip_multi_last_error()
    assert np.all(cent == SENTINEL) and np.all(q == SENTINEL)
    rc, cent, q = fit_call(vaqlib.vaqhip_multi_lut_fit_quantiles, X.astype(np.float32), bits, eig, 3, (C.c_int * 3)(0, 0, 0))
    assert rc == EINVAL and np.all(cent == SENTINEL) and np.all(q == SENTINEL)
    rc, cent, q = fit_call(vaqlib.vaqhip_lut_fit_quantiles_u8, X, bits, eig, 0)
    assert rc == EINVAL and np.all(cent == SENTINEL) and np.all(q == SENTINEL)
    r = vaq_amd.VaqMultiRefiner([0] * 3, D)
    r.set_rows_u8(X)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        r.fit_quantiles(bits, eig)
    assert e.value.code == EINVAL
    r.close()
    check_sharded(vaqlib, D, n, 3, True)


def test_python_adapters(vaqlib):
    import vaq_amd
    D, n = 5, 1000
    X, bits = byte_rows(n, D), fit_bits(D)
    want_c, want_q = float_fit(n, D, True)
    cent, q = vaq_amd.lut_fit_quantiles_multi_u8([0, 0], X, bits, rotation(D))
    same_bits(q, want_q, "lut_fit_quantiles_multi_u8")
    same_bits(np.ascontiguousarray(cent.T), want_c, "lut_fit_quantiles_multi_u8")
    t = vaq_amd.last_lut_fit_multi_timing()
    assert t["rows"] == n and t["dims"] == D and t["n_devices"] == 2 and t["columns_ms"] > 0
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc, v.mEigenVectors = list(bits), rotation(D)
    for devices in (None, [0, 0, 0]):
        v.fitQuantiles_u8(X, projected=False, devices=devices)
        same_bits(v.centroidsMat, want_c, f"fitQuantiles_u8(devices={devices})")
        same_bits(v.mQuantiles, want_q, f"fitQuantiles_u8(devices={devices})")
    v.close()


# ---- encode across the shards ----
def equal(a, b):
    return np.array_equal(a.labels, b.labels) and np.array_equal(u32(a.distances), u32(b.distances))


@pytest.mark.parametrize("devices", [[0, 0, 0], [0]], ids=["g3", "g1"])
def test_sharded_encode(vaqlib, devices):
    """VaqHipMulti.encode_u8 / encode_add_u8 == encode / encode_add on the widened rows: codes, cut, and the answers at
    k = 1 and 10.  N = 1000 cuts 334 / 334 / 332; encode_chunk_rows = 100 gives every shard several chunks and a
    short last one"""
    from vaq_amd.index import VaqHipMulti
    N, D, n1 = 1000, 32, 800
    X = byte_rows(N, D)
    Xf = X.astype(np.float32)
    c = make_case(978, D, [8, 7, 6, 5], 0, 9, rotate=True, scale=60.0)
    Xq = np.random.default_rng(8).uniform(0, 255, size=(9, D)).astype(np.float32)
    for projected in (False, True):
        a = VaqHipMulti(devices, c["bits"], c["cents"], c["eig"])
        b = VaqHipMulti(devices, c["bits"], c["cents"], c["eig"])
        a.set_option("encode_chunk_rows", 100)
        want = b.encode(Xf[:n1], projected=projected, id_base=7, return_codes=True)
        got = a.encode_u8(X[:n1], projected=projected, id_base=7, return_codes=True)
        assert np.array_equal(got, want)
        want = b.encode_add(Xf[n1:], projected=projected, return_codes=True)
        got = a.encode_add_u8(X[n1:], projected=projected, return_codes=True)
        assert np.array_equal(got, want)
        assert a.info()["shard_rows"] == b.info()["shard_rows"] and a.info()["id_base"] == 7 and a.info()["N"] == N
        t = a.last_encode_timing()
        assert t["rows"] == N - n1 and t["n_devices"] == len(devices) and t["encode_ms"] > 0
        for k in (1, 10):
            assert equal(a.search(Xq, k), b.search(Xq, k)), (projected, k)
        a.close(), b.close()


@pytest.mark.parametrize("devices", [[0, 0, 0], [0]], ids=["g3", "g1"])
def test_sharded_encode_lut(vaqlib, devices):
    """encode_lut_u8 / encode_lut_add_u8 == their float twins, with a rotation (projected=False) and without a
    projection (projected=True: the widen-only path)"""
    from vaq_amd.index import VaqHipMulti
    N, D, n1 = 1000, 8, 800
    X = byte_rows(N, D)
    Xf = X.astype(np.float32)
    bits = [8, 6, 5, 4, 3, 2, 1, 7]
    eig = rotation(D)
    rc, cent, q = fit_call(vaqlib.vaqhip_lut_fit_quantiles_u8, X, bits, eig, 0)
    assert rc == 0
    Xq = np.random.default_rng(9).uniform(0, 255, size=(9, D)).astype(np.float32)
    for projected in (False, True):
        a = VaqHipMulti(devices, bits, sr.centroid_list(bits, cent), eig, sequential_sum=True)
        b = VaqHipMulti(devices, bits, sr.centroid_list(bits, cent), eig, sequential_sum=True)
        for x in (a, b):
            x.set_lut_quantiles(q)
            x.set_option("exact_ties", 1)
        a.set_option("encode_chunk_rows", 100)
        want = b.encode_lut(Xf[:n1], projected=projected, return_codes=True)
        got = a.encode_lut_u8(X[:n1], projected=projected, return_codes=True)
        assert np.array_equal(got, want)
        want = b.encode_lut_add(Xf[n1:], projected=projected, return_codes=True)
        got = a.encode_lut_add_u8(X[n1:], projected=projected, return_codes=True)
        assert np.array_equal(got, want)
        assert a.info()["shard_rows"] == b.info()["shard_rows"]
        for k in (1, 10):
            assert equal(a.search(Xq, k), b.search(Xq, k)), (projected, k)
        a.close(), b.close()


def test_end_to_end_from_a_byte_refiner(vaqlib):
    """byte refiner -> fit_quantiles -> set_lut_quantiles -> encode_lut_from_refiner -> search_refine equals the same
    chain on a float refiner over the widened rows"""
    import vaq_amd
    from vaq_amd.index import VaqHipMulti
    N, D = 1000, 8
    X = byte_rows(N, D)
    bits = [8, 6, 5, 4, 3, 2, 1, 7]
    eig = rotation(D)
    Xq = np.random.default_rng(10).uniform(0, 255, size=(9, D)).astype(np.float32)
    Xq[0] = X[N // 2]
    devices = [0, 0, 0]
    out = []
    for rows, setter in ((X, "set_rows_u8"), (X.astype(np.float32), "set_rows")):
        r = vaq_amd.VaqMultiRefiner(devices, D)
        getattr(r, setter)(rows, id_base=3)
        cent, q = r.fit_quantiles(bits, eig)
        m = VaqHipMulti(devices, bits, sr.centroid_list(bits, np.ascontiguousarray(cent.T)), eig, sequential_sum=True)
        m.set_lut_quantiles(q)
        m.set_option("exact_ties", 1)
        r.exact_ties = True
        codes = m.encode_lut_from_refiner(r, return_codes=True)
        ans = m.search_refine(Xq, 100, 10, r)
        out.append((cent, q, codes, ans))
        m.close(), r.close()
    (c8, q8, codes8, a8), (cf, qf, codesf, af) = out
    same_bits(q8, qf, "quantiles")
    same_bits(c8, cf, "centres")
    assert np.array_equal(codes8, codesf) and len(np.unique(codes8)) > 8
    assert equal(a8, af) and a8.labels.min() >= 3


# ---- the C++ adapter and the demo ----
def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/build_u8_shim_test.cpp: VaqHip::encode(RowMatrix<uint8_t>) and
    BitVecEngineHip::binaryEncodingLUT(RowMatrix<uint8_t>), on one device and after setDevices(), against the float
    overloads"""
    from vaq_amd import build
    N, M, L, bits, nq = 3000, 8, 4, 8, 9
    D = M * L
    c = make_case(735, D, [bits] * M, 0, nq, rotate=True, scale=60.0)
    base = byte_rows(N, D)
    engine_bits = np.random.default_rng(12).integers(1, 9, size=D).astype(np.int32)
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([N, M, L, bits, nq], np.int32).tobytes())
        for cent in c["cents"]:
            f.write(np.ascontiguousarray(cent + 100, np.float32).tobytes())
        f.write(np.ascontiguousarray(c["eig"], np.float32).tobytes())
        f.write(base.tobytes())
        f.write(np.ascontiguousarray(c["X"] + 128, np.float32).tobytes())
        f.write(engine_bits.tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "build_u8_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "build_u8_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "build_u8_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_encodes_from_bvecs(vaqlib, tmp_path):
    """demo_vaqhip --file-format-ori bvecs --encode on a bvecs file == the fvecs run of the same vectors: the codebook
    and the answers; on one device and with --devices 0,0; and --lut-bits the same"""
    from vaq_amd import build, io
    exe = build.build_demo()
    N, M, L, nq, k = 1000, 8, 4, 9, 10
    D = M * L
    c = make_case(736, D, [8] * M, 0, nq, rotate=True, scale=60.0)
    X = byte_rows(N, D)
    Xq = np.random.default_rng(11).integers(0, 256, size=(nq, D), dtype=np.uint8)
    io.write_vecs(str(tmp_path / "base.bvecs"), X)
    io.write_vecs(str(tmp_path / "base.fvecs"), X.astype(np.float32))
    io.write_vecs(str(tmp_path / "q.bvecs"), Xq)
    io.write_vecs(str(tmp_path / "q.fvecs"), Xq.astype(np.float32))
    io.save_centroids([np.ascontiguousarray(cc + 100, np.float32) for cc in c["cents"]], str(tmp_path / "cent.bin"))
    np.ascontiguousarray(c["eig"], np.float32).tofile(str(tmp_path / "eig.f32"))
    lut_bits = ",".join(str(int(b)) for b in np.random.default_rng(13).integers(1, 9, size=D))

    def run(fmt, what, extra):
        tag = f"{fmt}_{what}_{len(extra)}"
        head = ["--encode", "--centroids", str(tmp_path / "cent.bin")] if what == "encode" else ["--lut-bits", lut_bits, "--exact-ties", "1"]
        r = subprocess.run([exe] + head + ["--eigen", str(tmp_path / "eig.f32"), "--dataset", str(tmp_path / f"base.{fmt}"),
                                           "--queries", str(tmp_path / f"q.{fmt}"), "--file-format-ori", fmt,
                                           "--timeseries-size", str(D), "--k", str(k), "--result", str(tmp_path / f"{tag}.csv"),
                                           "--save-enc", str(tmp_path / f"{tag}.cb")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout, io.load_codebook(str(tmp_path / f"{tag}.cb")), np.loadtxt(str(tmp_path / f"{tag}.csv"), delimiter=",", dtype=np.int64)

    for what in ("encode", "lut"):
        _, want_cb, want_ans = run("fvecs", what, [])
        assert want_cb.shape[0] == N and len(np.unique(want_cb)) > 8
        for extra in ([], ["--devices", "0,0"]):
            out, cb, ans = run("bvecs", what, extra)
            assert "byte rows" in out, out
            assert np.array_equal(cb, want_cb), (what, extra)
            assert np.array_equal(ans, want_ans), (what, extra)
