"""The encode across the shards of a multi-device index on the GPU (vaqhip_multi_encode_set_codes, _add_codes,
_from_refiner; vaq_amd/csrc/vaqhip_multi_encode.cpp).  Every case compares three routes with np.array_equal:
  (a) the new call on a multi index;
  (b) vaqhip_encode on a single index, then vaqhip_multi_set_codes_u16 (add_codes_u16) on a second multi index;
  (c) the oracle's encoder, for the codes.
codes_out, shard_rows, and the labels and distance BIT PATTERNS of later searches must agree.  Logical shards ([0] * G)
exercise every path on one GPU.  Nothing here has a tolerance: a row's code depends on that row and the codebooks only,
so the sharded answer is the single one."""
import functools
import os
import subprocess

import numpy as np
import pytest

from helpers import make_case

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
HEAP, EA, TI, FAST = 0x80, 0x02, 0x04, 0x08
KS = (1, 10, 100)
CONFIGS = {  # name: D, bits, rotation and projected = 0
    "d32_m8": (32, [8] * 8, False),
    "d48_m4_mixed": (48, [6, 5, 4, 3], False),
    "d128_m16_eig": (128, [8] * 16, True),
}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def config(name, n=1027):
    """codebooks, queries, a rotation when asked for, and n raw rows: gaussian, a fifth of them copies of other rows (equal
    codes, equal distances) and some the exact midpoint of two centroids (the strict `<` decides)"""
    D, bits, rotate = CONFIGS[name]
    c = make_case(4100 + D, D, bits, 0, 9, rotate=rotate)
    rng = np.random.default_rng(D)
    X = (rng.normal(size=(n, D)) * 30).astype(np.float32)
    if not rotate:
        L = c["L"]
        for i in range(0, min(n, 40), 2):
            s = i % c["M"]
            a, b = rng.integers(0, 1 << bits[s], 2)
            X[i, s * L:(s + 1) * L] = (c["cents"][s][a] + c["cents"][s][b]) * np.float32(0.5)
    X[rng.integers(0, n, n // 5)] = X[rng.integers(0, n, n // 5)]
    c["rows"] = np.ascontiguousarray(X)
    c["projected"] = not rotate
    return c


def single(c, seq=False):
    import vaq_amd
    v = vaq_amd.VaqHip(sequential_sum=seq)
    v.mBitsAlloc = c["bits"]
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    return v


def multi(c, G, method=HEAP | EA, visit=1.0, seq=False):
    from vaq_amd.index import VaqHipMulti
    m = VaqHipMulti([0] * G, c["bits"], c["cents"], c["eig"], sequential_sum=seq)
    if method:
        m.set_method(method, visit)
    return m


def host_codes(v, X, projected):
    v.encode(X, projected=projected)
    return np.array(v.mCodebook)


def cut_rows(N, G):
    per = -(-N // G)
    return [min(N, (g + 1) * per) - min(N, g * per) for g in range(G)]


def same_search(a, b, Q, ks=KS, what=""):
    for k in ks:
        ra, rb = a.search(Q, k), b.search(Q, k)
        assert np.array_equal(ra.labels, rb.labels), (what, k)
        assert np.array_equal(u32(ra.distances), u32(rb.distances)), (what, k)
    return ra


def same_state(a, b, what=""):
    ia, ib = a.info(), b.info()
    for key in ("N", "id_base", "shard_rows", "n_devices"):
        assert ia[key] == ib[key], (what, key, ia[key], ib[key])


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_shapes(vaqlib, oracle, name, G):
    """N in {1, G - 1, G, G + 1, 1000, 1027}: empty shards, one-row shards, an uneven last shard; HEAP|EA at k in
    {1, 10, 100} (N < k: the slots past N are -1 / FLT_MAX on both sides).  One pair of indexes serves every N, so
    each call also replaces what the call before left."""
    c = config(name)
    v, a, b = single(c), multi(c, G), multi(c, G)
    Xp = oracle.project(c["rows"], c["eig"]) if c["eig"] is not None else c["rows"]
    want_all = oracle.encode(Xp, c["cents"], nthreads=4)
    for N in sorted({1, G - 1, G, G + 1, 1000, 1027}):
        X = c["rows"][:N]
        got = a.encode(X, projected=c["projected"], id_base=7, return_codes=True)
        codes = host_codes(v, X, c["projected"]) if N else np.empty((0, c["M"]), np.uint16)
        b.set_codes(codes, id_base=7)
        assert np.array_equal(got, codes) and np.array_equal(got, want_all[:N]), (name, G, N)
        assert a.info()["shard_rows"] == cut_rows(N, G) and a.info()["N"] == N
        same_state(a, b, (name, G, N))
        last = same_search(a, b, c["X"], what=(name, G, N))
        lab = last.labels.reshape(len(c["X"]), KS[-1])
        assert np.all(lab[:, :min(N, 100)] >= 7) and np.all(lab[:, N:] == -1)
        t = a.last_encode_timing()
        assert t["rows"] == N and t["n_devices"] == G and t["total_ms"] > 0
        assert (t["encode_ms"] > 0 and t["set_codes_ms"] > 0) if N else (t["encode_ms"] == 0 and t["set_codes_ms"] == 0)
        # the two phases follow each other, each timed from its own start on the shard's stream: the slowest shard of
        # one plus the slowest of the other fit into the call
        assert t["encode_ms"] + t["set_codes_ms"] <= t["total_ms"], t
    # without codes_out nothing else changes
    assert a.encode(c["rows"], projected=c["projected"], id_base=7) is None
    b.set_codes(host_codes(v, c["rows"], c["projected"]), id_base=7)
    same_search(a, b, c["X"], what=(name, G, "no codes_out"))
    for x in (a, b, v):
        x.close()


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("chunk", [100, 256])
def test_chunk_edges(vaqlib, chunk, G):
    """N = 1027: with chunks of 100 and 256 rows the shard slices (1027; 343 + 343 + 341) end inside a chunk and one
    row past its edge (1027 = 4 * 256 + 3, 341 = 3 * 100 + 41, 343 = 256 + 87); a slice of exactly one and two chunks
    (N = chunk * G, 2 * chunk * G) ends on the edge.  Codes and answers are those of the default chunk."""
    for name in ("d32_m8", "d128_m16_eig"):
        c = config(name, 2 * 256 * 3)
        a, b = multi(c, G), multi(c, G)
        a.set_option("encode_chunk_rows", chunk)
        for N in (1027, chunk * G, 2 * chunk * G, chunk * G + 1):
            X = c["rows"][:N]
            got = a.encode(X, projected=c["projected"], return_codes=True)
            want = b.encode(X, projected=c["projected"], return_codes=True)
            assert np.array_equal(got, want), (name, chunk, G, N)
            same_state(a, b)
            same_search(a, b, c["X"], ks=(10,), what=(name, chunk, G, N))
        a.set_option("encode_chunk_rows", 0)  # back to the default
        assert np.array_equal(a.encode(X, projected=c["projected"], return_codes=True), want)
        a.close(), b.close()


@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_appends(vaqlib, oracle, G):
    """encode(600 rows, id_base 1 000 000), then encode_add of 1 row and of 300 rows == set_codes + add_codes twice with
    the host's codes; the last shard grows"""
    import vaq_amd
    for name in ("d48_m4_mixed", "d128_m16_eig"):
        c = config(name)
        X, p = c["rows"], c["projected"]
        v, a, b = single(c), multi(c, G), multi(c, G)
        with pytest.raises(vaq_amd.VaqHipError) as e:
            a.encode_add(X[:5], projected=p)
        assert e.value.code == -7 and a.info()["N"] == 0  # VAQHIP_ESTATE: no codes yet
        with pytest.raises(vaq_amd.VaqHipError) as e:
            a.set_codes(np.zeros((20, c["M"]), np.uint16), id_base=2**31 - 10)
        assert e.value.code == -6
        with pytest.raises(vaq_amd.VaqHipError) as e:
            a.encode_add(X[:5], projected=p)
        assert e.value.code == -7  # a set_codes that failed has given the shards no codes
        Xp = oracle.project(X, c["eig"]) if c["eig"] is not None else X
        want = oracle.encode(Xp, c["cents"], nthreads=4)
        got = [a.encode(X[:600], projected=p, id_base=1_000_000, return_codes=True)]
        b.set_codes(host_codes(v, X[:600], p), id_base=1_000_000)
        before = a.info()["shard_rows"]
        for lo, hi in ((600, 601), (601, 901)):
            got.append(a.encode_add(X[lo:hi], projected=p, return_codes=True))
            b.add_codes(host_codes(v, X[lo:hi], p))
            same_state(a, b, (name, G, hi))
            same_search(a, b, c["X"], what=(name, G, hi))
        assert np.array_equal(np.concatenate(got), want[:901])
        after = a.info()["shard_rows"]
        assert after[:-1] == before[:-1] and after[-1] == before[-1] + 301 and a.info()["N"] == 901
        t = a.last_encode_timing()
        assert a.info()["id_base"] == 1_000_000 and t["rows"] == 300
        assert 0 < t["encode_ms"] and 0 < t["set_codes_ms"] and t["encode_ms"] + t["set_codes_ms"] <= t["total_ms"], t
        assert a.encode_add(X[:0], projected=p, return_codes=True).shape == (0, c["M"]) and a.info()["N"] == 901
        # labels that would pass int32: what set_codes returns for the same N and id_base, and nothing has changed
        for x in (a, b):
            with pytest.raises(vaq_amd.VaqHipError) as e:
                x.encode(X[:20], projected=p, id_base=2**31 - 10) if x is a else x.set_codes(want[:20], id_base=2**31 - 10)
            assert e.value.code == -6  # VAQHIP_ERANGE
        assert a.info()["N"] == 901 and a.info()["shard_rows"] == after
        for x in (a, b, v):
            x.close()


def decoded_rows(z):
    """the rows (in PCA space) whose codes are the fixture's: the centroids of their codes"""
    M = len(z["bits"])
    return np.ascontiguousarray(np.concatenate([z[f"cent{s}"][z["codes"][:, s]] for s in range(M)], axis=1), np.float32)


def test_exact_ties_sees_no_difference(vaqlib):
    """"exact_ties" = 1 on the integer tie data of d16_m4_b3_ties.npz, rows = the decoded codes: the chain over the
    shards runs over the rows the shards encoded themselves"""
    z = np.load(os.path.join(GOLD, "d16_m4_b3_ties.npz"))
    c = dict(bits=[int(x) for x in z["bits"]], cents=[z[f"cent{s}"] for s in range(4)], eig=z["eig"], M=4)
    rows = decoded_rows(z)
    v = single(c)
    codes = host_codes(v, rows, True)
    for G in (2, 3, 8):
        a, b = multi(c, G), multi(c, G)
        for m in (a, b):
            m.set_option("exact_ties", 1)
        assert np.array_equal(a.encode(rows, projected=True, return_codes=True), codes)
        b.set_codes(codes)
        r = same_search(a, b, z["X"], what=("exact_ties", G))
        d = r.distances.reshape(len(z["X"]), -1)
        assert (d[:, 1:] == d[:, :-1]).sum() > 100  # equal neighbours: the chain had work to do
        a.close(), b.close()
    v.close()


def test_fast_sees_no_difference(vaqlib):
    """FAST on 4-bit codes after set_lut_quantization, before and after the encode"""
    c = make_case(4400, 32, [4] * 8, 0, 9, rotate=False)
    rows = (np.random.default_rng(44).normal(size=(1027, 32)) * 30).astype(np.float32)
    L = c["L"]
    lut = np.stack([((c["X"][:, None, s * L:(s + 1) * L] - c["cents"][s][None]) ** 2).sum(-1) for s in range(8)], 1)
    off = lut.min(axis=(0, 2)).astype(np.float32)
    sc = (np.float32(230) / (lut.max(axis=(0, 2)) - lut.min(axis=(0, 2)))).astype(np.float32)
    v = single(c)
    codes = host_codes(v, rows, True)
    for G in (1, 3, 8):
        a, b = multi(c, G, method=0), multi(c, G, method=0)
        for m in (a, b):
            m.set_lut_quantization(off, sc)
            m.set_method(FAST)
        a.encode(rows, projected=True)
        b.set_codes(codes)
        same_search(a, b, c["X"], what=("fast", G))
        a.encode_add(rows[:50], projected=True)
        b.add_codes(codes[:50])
        same_search(a, b, c["X"], what=("fast append", G))
        a.close(), b.close()
    v.close()


def test_ti_and_kmeans_see_no_difference(vaqlib):
    """set_ti_clusters once before and once after the encode, TI|EA at visit 0.25 and 1; cluster_ti_kmeans centres"""
    c = config("d32_m8")
    rows = c["rows"]
    v = single(c)
    codes = host_codes(v, rows, True)
    seg, T = 4, 16
    pick = np.random.default_rng(3).integers(0, len(rows), T)
    clusters = np.ascontiguousarray(np.concatenate([c["cents"][s][codes[pick, s]] for s in range(seg)], axis=1))
    for G in (2, 3):
        for visit in (0.25, 1.0):
            before, after, b = multi(c, G, 0), multi(c, G, 0), multi(c, G, 0)
            before.set_ti_clusters(clusters, seg)
            before.encode(rows, projected=True)
            after.encode(rows, projected=True)
            after.set_ti_clusters(clusters, seg)
            b.set_codes(codes)
            b.set_ti_clusters(clusters, seg)
            for m in (before, after, b):
                m.set_method(TI | EA, visit)
            same_search(before, b, c["X"], what=("ti before", G, visit))
            same_search(after, b, c["X"], what=("ti after", G, visit))
            for m in (before, after, b):
                m.close()
        a, b = multi(c, G), multi(c, G)
        a.encode(rows, projected=True)
        b.set_codes(codes)
        ca, ita, na = a.cluster_ti_kmeans(T, seg, 10)
        cb, itb, nb = b.cluster_ti_kmeans(T, seg, 10)
        assert np.array_equal(u32(ca), u32(cb)) and (ita, na) == (itb, nb)
        for m in (a, b):
            m.set_method(TI | EA, 0.5)
        same_search(a, b, c["X"], what=("after kmeans", G))
        a.close(), b.close()
    v.close()


def test_awkward_rows(vaqlib):
    """a row with a NaN coordinate, one with +inf, one all zero, among ordinary rows: the codes are vaqhip_encode's,
    whatever they are -- on a plain index, on a rotated one (projected = 0) and on a VAQHIP_SUM_SEQUENTIAL index with
    projected = 0, whose checked projection turns non-finite coordinates into 0"""
    def planted(X):
        X = X.copy()
        X[3, 1] = np.nan
        X[170, 0] = np.inf
        X[171, -1] = -np.inf
        X[340] = 0
        X[-1, 2] = np.nan
        return X

    for name in ("d32_m8", "d128_m16_eig"):
        c = config(name)
        X = planted(c["rows"][:400])
        v, a, b = single(c), multi(c, 3), multi(c, 3)
        codes = host_codes(v, X, c["projected"])
        assert np.array_equal(a.encode(X, projected=c["projected"], return_codes=True), codes)
        b.set_codes(codes)
        same_search(a, b, c["X"], ks=(10,), what=name)
        for x in (a, b, v):
            x.close()
    rng = np.random.default_rng(8)
    D = 8
    c = dict(bits=[4] * D, M=D, cents=[np.sort(rng.normal(size=(16, 1)).astype(np.float32) * 30, axis=0) for _ in range(D)],
             eig=np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32))
    X = planted((rng.normal(size=(400, D)) * 30).astype(np.float32))
    Q = (rng.normal(size=(5, D)) * 30).astype(np.float32)
    v, a, b = single(c, seq=True), multi(c, 3, method=HEAP, seq=True), multi(c, 3, method=HEAP, seq=True)
    codes = host_codes(v, X, False)
    assert np.array_equal(a.encode(X, projected=False, return_codes=True), codes)
    b.set_codes(codes)
    same_search(a, b, Q, ks=(1, 10), what="sequential")
    for x in (a, b, v):
        x.close()


@pytest.mark.parametrize("G", [2, 3, 8])
def test_from_refiner(vaqlib, oracle, G):
    """VaqMultiRefiner.set_rows(X[:700], id_base = 1 000 000) + add_rows(X[700:1027]), then encode_from_refiner: the
    codes of vaqhip_encode(projected = 0) over X, the refiner's shard_rows, and search_refine equal to the host-code
    route (set_codes of 700 + add_codes of 327, the same cut) slot for slot"""
    import vaq_amd
    c = config("d128_m16_eig")
    X, D = c["rows"], 128
    r = vaq_amd.VaqMultiRefiner([0] * G, D)
    a, b, v = multi(c, G), multi(c, G), single(c)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        a.encode_from_refiner(r)
    assert e.value.code == -7  # VAQHIP_ESTATE: a refiner without rows
    r.set_rows(X[:700], id_base=1_000_000)
    r.add_rows(X[700:])
    got = a.encode_from_refiner(r, return_codes=True)
    codes = host_codes(v, X, False)
    assert np.array_equal(got, codes)
    assert np.array_equal(got, oracle.encode(oracle.project(X, c["eig"]), c["cents"], nthreads=4))
    b.set_codes(codes[:700], id_base=1_000_000)
    b.add_codes(codes[700:])
    same_state(a, b)
    assert a.info()["shard_rows"] == r.info()["shard_rows"] == cut_rows(700, G)[:-1] + [cut_rows(700, G)[-1] + 327]
    t = a.last_encode_timing()
    assert t["rows"] == 1027 and t["encode_ms"] > 0 and t["set_codes_ms"] > 0
    assert t["encode_ms"] + t["set_codes_ms"] <= t["total_ms"], t
    same_search(a, b, c["X"], what=("refiner", G))
    for exact in (False, True):
        r.exact_ties = exact
        fa, fb = a.search_refine(c["X"], 100, 10, r), b.search_refine(c["X"], 100, 10, r)
        assert np.array_equal(fa.labels, fb.labels) and np.array_equal(u32(fa.distances), u32(fb.distances))
        assert fa.labels.min() >= 1_000_000
    assert a.encode_from_refiner(r) is None  # again, without codes_out
    same_search(a, b, c["X"], ks=(10,), what=("refiner again", G))
    # an empty shard: 2 rows on G >= 3 shards
    r.set_rows(X[:2], id_base=5)
    assert np.array_equal(a.encode_from_refiner(r, return_codes=True), codes[:2])
    assert a.info()["shard_rows"] == r.info()["shard_rows"] and a.info()["id_base"] == 5
    b.set_codes(codes[:2], id_base=5)
    same_search(a, b, c["X"], ks=(10,), what=("refiner 2 rows", G))
    # mismatched device lists or D: EINVAL, and the index keeps its rows
    others = [vaq_amd.VaqMultiRefiner([0] * (G + 1), D), vaq_amd.VaqMultiRefiner([0] * G, D + 1)]
    others[0].set_rows(X[:10])
    others[1].set_rows(np.zeros((10, D + 1), np.float32))
    for o in others:
        with pytest.raises(vaq_amd.VaqHipError) as e:
            a.encode_from_refiner(o)
        assert e.value.code == -1
        o.close()
    assert a.info()["N"] == 2
    for x in (a, b, v, r):
        x.close()


def test_state_and_device(vaqlib):
    """the caller's current device is what it was after a success and after a refused call; growing then shrinking N.
    The shards live on device 0 and the caller sits on the LAST device of the machine, so on a machine with several
    GPUs a call that left the shard's device current is caught; with one GPU the device can only be 0 and this part of
    the test cannot fail (the restore is DeviceGuard's, vaqhip_dev.h, as in every other multi entry point)."""
    import torch
    import vaq_amd
    c = config("d32_m8")
    a, b, v = multi(c, 3), multi(c, 3), single(c)
    current = torch.cuda.current_device
    torch.cuda.set_device(torch.cuda.device_count() - 1)
    dev = current()
    for N in (300, 1027, 40):
        assert np.array_equal(a.encode(c["rows"][:N], return_codes=True), host_codes(v, c["rows"][:N], True))
        assert current() == dev
        b.set_codes(np.array(v.mCodebook))
        same_state(a, b)
        same_search(a, b, c["X"], what=N)
    with pytest.raises(vaq_amd.VaqHipError):
        a.encode(c["rows"][:20], id_base=2**31 - 10)
    with pytest.raises(vaq_amd.VaqHipError):
        a.encode(np.zeros((4, 31), np.float32))
    assert vaqlib.vaqhip_multi_encode_set_codes(a._h, None, 5, 1, 0, None) == -1
    assert current() == dev and a.info()["N"] == 40
    same_search(a, b, c["X"], ks=(10,), what="after refusals")
    torch.cuda.set_device(0)
    for x in (a, b, v):
        x.close()


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/encode_multi_shim_test.cpp: VaqHip::encode after setDevices({0, 0, 0}) and encodeRefineDataset() give
    the single device's mCodebook and search() answers"""
    from vaq_amd import build
    N, M, L, bits, nq = 3001, 8, 4, 8, 9
    c = make_case(833, M * L, [bits] * M, 0, nq, rotate=True)
    rng = np.random.default_rng(5)
    base = (rng.normal(size=(N, M * L)) * 30).astype(np.float32)
    base[rng.integers(0, N, 600)] = base[rng.integers(0, N, 600)]
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([N, M, L, bits, nq], np.int32).tobytes())
        for cent in c["cents"]:
            f.write(np.ascontiguousarray(cent, np.float32).tobytes())
        f.write(np.ascontiguousarray(c["eig"], np.float32).tobytes())
        f.write(base.tobytes())
        f.write(np.ascontiguousarray(c["X"], np.float32).tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "encode_multi_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "encode_multi_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "encode_multi_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_encodes_across_the_shards(vaqlib, tmp_path):
    """demo_vaqhip --encode over the siftsmall queries and a sift-like base: the run with --devices 0,0
    --refine-resident (the rows uploaded once and encoded where they lie) and the run with --devices 0,0 alone (every
    shard encodes its slice) print the recall lines and write the codebook of the run without the two flags"""
    import torch
    from vaq_amd import build, harness, io
    exe = build.build_demo()
    N, D, k = 10_000, 128, 100
    q_h = io.read_fvecs(os.path.join(GOLD, "siftsmall", "siftsmall_query.fvecs")).astype(np.float32)
    bits = [8] * 8
    base = harness.sift_like(N, D, stream=0, device="cuda")
    E = harness.pca_eigenvectors(base)
    cents = harness.train_codebooks(base @ E.to("cuda"), bits, iters=4)
    base_h = base.cpu().numpy()
    del base
    torch.cuda.empty_cache()
    io.save_centroids(cents, str(tmp_path / "c.bin"))
    E.numpy().astype(np.float32).tofile(str(tmp_path / "e.f32"))
    io.write_vecs(str(tmp_path / "base.fvecs"), base_h)
    io.write_vecs(str(tmp_path / "q.fvecs"), q_h)
    d = ((q_h[:, None, :].astype(np.float64) - base_h[None, :, :]) ** 2).sum(-1)
    io.write_vecs(str(tmp_path / "gt.ivecs"), np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32))
    common = [exe, "--centroids", str(tmp_path / "c.bin"), "--eigen", str(tmp_path / "e.f32"), "--encode",
              "--dataset", str(tmp_path / "base.fvecs"), "--queries", str(tmp_path / "q.fvecs"), "--timeseries-size", "128",
              "--queries-size", str(len(q_h)), "--method", "VAQ64m8min8max8var1,HEAP", "--k", str(k),
              "--groundtruth", str(tmp_path / "gt.ivecs")]
    outs, books = [], []
    for i, extra in enumerate(([], ["--devices", "0,0"], ["--devices", "0,0", "--refine-resident"])):
        r = subprocess.run(common + extra + ["--save-enc", str(tmp_path / f"cb{i}.bin")], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        assert "== Encoding time" in r.stdout
        assert ("across 2 shards: total" in r.stdout) == bool(extra), r.stdout
        assert ("from the resident rows" in r.stdout) == (len(extra) == 3), r.stdout
        outs.append([x for x in r.stdout.splitlines() if "precision(avg_recall)" in x or "recall@R" in x])
        books.append(open(tmp_path / f"cb{i}.bin", "rb").read())
    assert len(outs[0]) == 2 and outs[0] == outs[1] == outs[2], outs
    assert float(outs[0][0].split(":")[1]) > 0.1
    assert books[0] == books[1] == books[2]
