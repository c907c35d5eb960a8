"""vaqhip_multi_cluster_ti_kmeans on the GPU: the k-means of VAQ::clusterTI(true) over the shards of a multi-device
index -- the reference's centres (fixtures: tests/golden/kmeans/README.md) for any number of shards, through the
C ABI, the Python mirror and the C++ adapter, and the TI search on the centres it leaves.  Logical shards on
device 0 everywhere; where the machine has two GPUs the fixture cases also run spread over both."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import kmeans_ref as kr
from helpers import assert_topk_matches

pytestmark = pytest.mark.gpu
E2E_CASE = "n70000_s2_l16_t64"  # converges, no NaN centre, byte-code layout


def _bits(ncent):
    return int(ncent).bit_length() - 1


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return kr.make_inputs(name)


def _devices(G, spread):
    """G shards on device 0, or dealt over devices 0 and 1 (skipped where there is one GPU)."""
    if spread == "one_gpu":
        return [0] * G
    from vaq_amd import _lib
    if _lib.load().vaqhip_device_count() < 2:
        pytest.skip("needs two GPUs")
    return [g % 2 for g in range(G)]


def _multi(name, devices, codes=None, id_base=0, sequential_sum=False):
    from vaq_amd.index import VaqHipMulti
    N, seg, L, T, ncent, M = kr.CASES[name]
    all_codes, cents = _inputs(name)
    m = VaqHipMulti(devices, [_bits(ncent)] * M, cents, sequential_sum=sequential_sum)
    if codes is not False:
        m.set_codes(all_codes if codes is None else codes, id_base)
    return m


def _kmeans(m, T, seg, max_iter=kr.MAX_ITER, want_out=True):
    from vaq_amd import _lib
    out = np.full((max(T, 0), max(seg, 0) * (m.D // m.M)), -1.0, np.float32)
    iters, nan_rows = C.c_int(-1), C.c_int(-1)
    rc = _lib.load().vaqhip_multi_cluster_ti_kmeans(m._h, T, seg, max_iter,
                                                    out.ctypes.data_as(C.c_void_p) if want_out else None,
                                                    C.byref(iters) if want_out else None,
                                                    C.byref(nan_rows) if want_out else None)
    return rc, out, iters.value, nan_rows.value


def _shard_info(m, g):
    from vaq_amd import _lib
    inf = _lib.Info()
    assert _lib.load().vaqhip_index_info(C.c_void_p(m.shard(g)), C.byref(inf)) == 0
    return inf


# sampled, 25 600 rows: slices of 8 534 end inside a workgroup tile, the half boundary lies in the middle slice,
# and the summation order decides the centres / sampled, byte layout / all rows, odd N, bit-packed / 512-dim rows:
# the assign form that reads X from global memory / empty clusters, runs to the cap / one shard
FIXTURE_CASES = [("n40000_s4_l16_t100", 3), ("n70000_s2_l16_t64", 2), ("n70000_s2_l16_t64", 5),
                 ("n4001_s5_l8_t24", 3), ("n301_s4_l128_t7", 4), ("n20000_s1_l20_t50", 2), ("n5000_s3_l4_t37", 1)]


@pytest.mark.parametrize("spread", ["one_gpu", "two_gpus"])
@pytest.mark.parametrize("name,G", FIXTURE_CASES, ids=[f"{n}-G{g}" for n, g in FIXTURE_CASES])
def test_centres_equal_the_reference(vaqlib, name, G, spread):
    if G == 1 and spread == "two_gpus":
        pytest.skip("one shard has one device")
    N, seg, L, T, ncent, M = kr.CASES[name]
    fx = kr.load_fixture(name)
    m = _multi(name, _devices(G, spread))
    assert _shard_info(m, 0).layout == (0 if (ncent, M) == (256, 8) else 1)
    rc, out, iters, nan_rows = _kmeans(m, T, seg)
    assert rc == 0, vaqlib.vaqhip_multi_last_error()
    print(f"{name} G={G}: iterations {iters} (reference {int(fx['iterations'])}), NaN centres {nan_rows} "
          f"(reference {int(fx['nan_rows'].sum())})")
    kr.assert_centres_equal(out, fx["centres"], f"{name} G={G}")
    assert iters == int(fx["iterations"])
    assert nan_rows == int(fx["nan_rows"].sum())
    for g in range(G):
        inf = _shard_info(m, g)
        assert (inf.ti_clusters, inf.ti_segments) == (T, seg) and inf.methods & 0x04
    t = m.last_kmeans_timing()
    assert (t["iterations"], t["rows"], t["dims"], t["clusters"]) == (iters, min(N, 256 * T), seg * L, T)
    assert t["total_ms"] > 0 and t["assign_ms"] == 0  # (the phases are timed only with option "timing")
    m.close()


@pytest.mark.parametrize("spread", ["one_gpu", "two_gpus"])
def test_empty_shard_and_tiny_n(vaqlib, spread):
    """N = 9 over four shards (3, 3, 3, 0 rows), T = 4: the single index's centres, and the NumPy restatement's."""
    from vaq_amd.index import VaqHip, VaqHipMulti
    N, M, L, ncent, T, seg = 9, 4, 4, 8, 4, 2
    rng = np.random.default_rng(909)
    cents = [rng.normal(size=(ncent, L)).astype(np.float32) for _ in range(M)]
    codes = rng.integers(0, ncent, size=(N, M)).astype(np.uint16)
    m = VaqHipMulti(_devices(4, spread), [3] * M, cents)
    m.set_codes(codes)
    assert m.info()["shard_rows"] == [3, 3, 3, 0]
    got, iters, nan_rows = m.cluster_ti_kmeans(T, seg)
    v = VaqHip()
    v.parseMethodString(f"VAQ12m4min3max3var1,EA_TI{T}m{seg}")
    v.mBitsAlloc = [3] * M
    v.mCentroidsPerSubs = cents
    v.mCodebook = codes
    v.clusterTI(True)
    kr.assert_centres_equal(got, v.mTIClusters, "single index")
    assert (iters, nan_rows) == (v.kmeansIterations, v.kmeansNanRows)
    want, want_iters, want_nan = kr.fit_codebook(codes, cents, seg, T)
    kr.assert_centres_equal(got, want, "kmeans_ref")
    assert (iters, nan_rows) == (want_iters, int(want_nan.sum()))
    m.close()
    v.close()


def test_after_add_codes(vaqlib):
    """The last shard grown by add_codes holds more rows than the others: the sample still finds every row."""
    name = "n4001_s5_l8_t24"
    N, seg, L, T, ncent, M = kr.CASES[name]
    codes, _ = _inputs(name)
    fx = kr.load_fixture(name)
    m = _multi(name, [0, 0, 0], codes[:3000])
    m.add_codes(codes[3000:])
    assert m.info()["shard_rows"] == [1000, 1000, 2001]
    rc, out, iters, nan_rows = _kmeans(m, T, seg)
    assert rc == 0, vaqlib.vaqhip_multi_last_error()
    kr.assert_centres_equal(out, fx["centres"], "after add_codes")
    assert (iters, nan_rows) == (int(fx["iterations"]), int(fx["nan_rows"].sum()))
    m.close()


def test_second_call_and_id_base(vaqlib):
    """A second call gathers through the TI-grouped shards' row order and gives the first call's centres; id_base
    plays no part in the sample."""
    name = "n40000_s4_l16_t100"  # sampled
    N, seg, L, T, ncent, M = kr.CASES[name]
    fx = kr.load_fixture(name)
    m = _multi(name, [0, 0, 0])
    rc, first, it1, _ = _kmeans(m, T, seg)
    assert rc == 0, vaqlib.vaqhip_multi_last_error()
    assert _shard_info(m, 1).ti_clusters == T
    rc, again, it2, _ = _kmeans(m, T, seg)
    assert rc == 0, vaqlib.vaqhip_multi_last_error()
    kr.assert_centres_equal(first, fx["centres"], "first call")
    kr.assert_centres_equal(again, first, "second call")
    assert it1 == it2 == int(fx["iterations"])
    m.close()
    b = _multi(name, [0, 0], id_base=1000)
    rc, based, it3, _ = _kmeans(b, T, seg)
    assert rc == 0, vaqlib.vaqhip_multi_last_error()
    kr.assert_centres_equal(based, fx["centres"], "id_base = 1000")
    assert it3 == int(fx["iterations"]) and b.info()["id_base"] == 1000
    b.close()


def test_search_after_kmeans_equals_the_single_index_and_the_oracle(vaqlib, oracle):
    """EA_TI on the shards the k-means grouped == on a single VaqHip after clusterTI(True) == the oracle's TI path."""
    from vaq_amd.index import NNMethod, VaqHip
    name = E2E_CASE
    N, seg, L, T, ncent, M = kr.CASES[name]
    codes, cents = _inputs(name)
    fx = kr.load_fixture(name)
    nq = 12
    X = (np.random.default_rng(71).normal(size=(nq, M * L)) * 1.5).astype(np.float32)

    m = _multi(name, [0, 0, 0])
    centres, iters, nan_rows = m.cluster_ti_kmeans(T, seg)
    kr.assert_centres_equal(centres, fx["centres"], "multi k-means")
    assert (iters, nan_rows) == (int(fx["iterations"]), 0)

    a = VaqHip()
    a.parseMethodString(f"VAQ{8 * M}m{M}min8max8var1,EA_TI{T}m{seg}")
    a.mBitsAlloc = [_bits(ncent)] * M
    a.mCentroidsPerSubs = cents
    a.mCodebook = codes
    a.clusterTI(True)

    ti = oracle.cluster_ti(codes, cents, np.ascontiguousarray(fx["centres"]), seg)
    for visit in (1.0, 0.25):
        a.mVisit = visit
        m.set_method(NNMethod.TI | NNMethod.EA, visit)
        for k in (1, 10):
            rm = m.search(X, k, projected=True)
            ra = a.search(X, k, projected=True)
            assert np.array_equal(rm.labels, ra.labels), (visit, k)
            assert np.array_equal(rm.distances.view(np.uint32), ra.distances.view(np.uint32)), (visit, k)
            ol, od, _ = oracle.search_ti(X, cents, ti, k, visit=visit, projected=True)
            assert_topk_matches(rm.labels.reshape(nq, k), rm.distances.reshape(nq, k), ol, od,
                                what=f"multi TI|EA after k-means visit={visit} k={k}")
    a.close()
    m.close()


def test_refusals(vaqlib):
    from vaq_amd.index import VaqHipMulti
    L = vaqlib
    name = "n2500_s1_l6_t10"
    N, seg, Ls, T, ncent, M = kr.CASES[name]
    codes, cents = _inputs(name)

    def refused(m, rc, want, G):
        assert rc == want
        assert L.vaqhip_multi_last_error()  # non-empty
        for g in range(G):
            assert _shard_info(m, g).ti_clusters == 0

    # before the codes are set: a state error
    m = _multi(name, [0, 0], codes=False)
    refused(m, _kmeans(m, T, seg)[0], -7, 2)
    assert b"codes" in L.vaqhip_multi_last_error()
    m.set_codes(codes[:100])
    # bad arguments
    refused(m, _kmeans(m, 101, seg)[0], -1, 2)          # T > N: the reference reads out of bounds
    refused(m, _kmeans(m, 0, seg)[0], -1, 2)
    refused(m, _kmeans(m, T, 0)[0], -1, 2)
    refused(m, _kmeans(m, T, M + 1)[0], -1, 2)
    refused(m, _kmeans(m, T, seg, max_iter=0)[0], -1, 2)
    assert L.vaqhip_multi_cluster_ti_kmeans(None, T, seg, 50, None, None, None) == -1
    assert L.vaqhip_multi_last_error()
    # the limits of set_ti_clusters
    refused(m, _kmeans(m, 4097, seg)[0], -2, 2)
    # the out-pointers may be NULL
    assert _kmeans(m, T, seg, want_out=False)[0] == 0
    assert [_shard_info(m, g).ti_clusters for g in range(2)] == [T, T]
    m.close()
    # centres of more than 1024 dims
    wide = VaqHipMulti([0, 0], [1] * 4, [np.zeros((2, 300), np.float32)] * 4)
    wide.set_codes(np.zeros((64, 4), np.uint16))
    refused(wide, _kmeans(wide, 2, 4)[0], -2, 2)
    wide.close()
    # a sequential-sum index: TI is a VAQ::search method
    sq = _multi(name, [0, 0], codes[:100], sequential_sum=True)
    refused(sq, _kmeans(sq, T, seg)[0], -1, 2)
    sq.close()


def test_cpp_adapter_cluster_ti_multi(tmp_path):
    """VaqHip::clusterTI(true) after setDevices({0, 0, 0}) (tests/cpp/kmeans_cluster_ti_multi_test.cpp)."""
    from vaq_amd import build
    name = "n5000_s3_l4_t37"
    N, seg, L, T, ncent, M = kr.CASES[name]
    codes, cents = _inputs(name)
    fx = kr.load_fixture(name)
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([N, M, L, _bits(ncent), T, seg, int(fx["iterations"]), int(fx["nan_rows"].sum())], np.int32).tobytes())
        f.write(np.ascontiguousarray(codes).tobytes())
        for c in cents:
            f.write(np.ascontiguousarray(c).tobytes())
        f.write(np.ascontiguousarray(fx["centres"], np.float32).tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "kmeans_cluster_ti_multi_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "kmeans_cluster_ti_multi_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "kmeans_cluster_ti_multi ok" in r.stdout, r.stdout + r.stderr
