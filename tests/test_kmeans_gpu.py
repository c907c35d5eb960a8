"""vaqhip_index_cluster_ti_kmeans on the GPU: the k-means of VAQ::clusterTI(true), centre for centre what the
reference computes (fixtures: tests/golden/kmeans/README.md), through the C ABI, the Python mirror and the
C++ adapter, and the TI search on the centres it leaves."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmeans_ref as kr
from helpers import assert_topk_matches

pytestmark = pytest.mark.gpu
CASES = list(kr.CASES)
E2E_CASE = "n70000_s2_l16_t64"  # converges, no NaN centre, byte-code layout


def _bits(ncent):
    return int(ncent).bit_length() - 1


def _index(name, codes=None):
    """A VaqHip over the case's codebooks with its codes on the device (exhaustive order)."""
    from vaq_amd.index import VaqHip
    N, seg, L, T, ncent, M = kr.CASES[name]
    all_codes, cents = kr.make_inputs(name)
    v = VaqHip()
    v.mBitsAlloc = [_bits(ncent)] * M
    v.mCentroidsPerSubs = cents
    v.mCodebook = all_codes if codes is None else codes
    v._ensure_codes()
    return v


def _kmeans(v, T, seg, max_iter=kr.MAX_ITER, want_out=True):
    from vaq_amd import _lib
    out = np.full((T, seg * v.mSubsLen), -1.0, np.float32)
    iters, nan_rows = C.c_int(-1), C.c_int(-1)
    rc = _lib.load().vaqhip_index_cluster_ti_kmeans(v._h, T, seg, max_iter, out.ctypes.data_as(C.c_void_p) if want_out else None,
                                                    C.byref(iters) if want_out else None,
                                                    C.byref(nan_rows) if want_out else None)
    return rc, out, iters.value, nan_rows.value


@pytest.mark.parametrize("name", CASES)
def test_centres_equal_the_reference(name):
    N, seg, L, T, ncent, M = kr.CASES[name]
    fx = kr.load_fixture(name)
    v = _index(name)
    assert v.info()["layout"] == (0 if (ncent, M) == (256, 8) else 1)  # byte codes / bit-packed: both occur
    rc, out, iters, nan_rows = _kmeans(v, T, seg)
    assert rc == 0
    print(f"{name}: iterations {iters} (reference {int(fx['iterations'])}), NaN centres {nan_rows} "
          f"(reference {int(fx['nan_rows'].sum())})")
    kr.assert_centres_equal(out, fx["centres"], name)
    assert iters == int(fx["iterations"])
    assert nan_rows == int(fx["nan_rows"].sum())
    info = v.info()
    assert (info["ti_clusters"], info["ti_segments"], info["N"]) == (T, seg, N)
    assert info["methods"] & 0x04
    v.close()


def test_both_layouts_are_covered():
    """(the index keeps one byte per code for 8, 16 or 32 subspaces of 8 bits, bit-packed rows otherwise)"""
    assert {kr.CASES[n][4:] == (256, 8) for n in CASES} == {True, False}


def test_search_after_kmeans_equals_set_ti_clusters_and_the_oracle(oracle):
    """EA_TI on the index the k-means grouped == on an index given the same centres == the oracle's TI path."""
    from vaq_amd.index import NNMethod, VaqHip
    name = E2E_CASE
    N, seg, L, T, ncent, M = kr.CASES[name]
    codes, cents = kr.make_inputs(name)
    fx = kr.load_fixture(name)
    assert not fx["nan_rows"].any() and int(fx["iterations"]) < kr.MAX_ITER
    nq = 12
    X = (np.random.default_rng(71).normal(size=(nq, M * L)) * 1.5).astype(np.float32)

    a = VaqHip()
    a.parseMethodString(f"VAQ{8 * M}m{M}min8max8var1,EA_TI{T}m{seg}")
    a.mBitsAlloc = [_bits(ncent)] * M
    a.mCentroidsPerSubs = cents
    a.mCodebook = codes
    a.clusterTI(True)
    kr.assert_centres_equal(a.mTIClusters, fx["centres"], "python clusterTI(True)")
    assert (a.kmeansIterations, a.kmeansNanRows) == (int(fx["iterations"]), 0)

    b = VaqHip()
    b.mBitsAlloc = [_bits(ncent)] * M
    b.mCentroidsPerSubs = cents
    b.mMethods = NNMethod.TI | NNMethod.EA
    b.mTISegmentNum, b.mTIClusterNum = seg, T
    b.mTIClusters = np.array(fx["centres"])
    b.mCodebook = codes

    ti = oracle.cluster_ti(codes, cents, np.ascontiguousarray(fx["centres"]), seg)
    for visit in (1.0, 0.25, 0.05):
        a.mVisit = b.mVisit = visit
        for k in (1, 10):
            ra = a.search(X, k, projected=True)
            rb = b.search(X, k, projected=True)
            assert np.array_equal(ra.labels, rb.labels), (visit, k)
            assert np.array_equal(ra.distances.view(np.uint32), rb.distances.view(np.uint32)), (visit, k)
            ol, od, _ = oracle.search_ti(X, cents, ti, k, visit=visit, projected=True)
            assert_topk_matches(ra.labels.reshape(nq, k), ra.distances.reshape(nq, k), ol, od,
                                what=f"TI|EA after k-means visit={visit} k={k}")
    a.close()
    b.close()


def test_cpp_adapter_cluster_ti(tmp_path):
    """VaqHip::clusterTI(true) of include/vaqhip.hpp (tests/cpp/kmeans_cluster_ti_test.cpp)."""
    from vaq_amd import build
    name = "n5000_s3_l4_t37"
    N, seg, L, T, ncent, M = kr.CASES[name]
    codes, cents = kr.make_inputs(name)
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
    exe = str(tmp_path / "kmeans_cluster_ti_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "kmeans_cluster_ti_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "kmeans_cluster_ti ok" in r.stdout, r.stdout + r.stderr


def test_refusals():
    from vaq_amd import _lib
    from vaq_amd.index import VaqHip
    L = _lib.load()
    name = "n2500_s1_l6_t10"
    N, seg, Ls, T, ncent, M = kr.CASES[name]
    codes, cents = kr.make_inputs(name)
    # before the codes are set: a state error
    v = VaqHip()
    v.mBitsAlloc = [_bits(ncent)] * M
    v.mCentroidsPerSubs = cents
    v._ensure_index()
    assert _kmeans(v, T, seg)[0] == -7
    assert b"codes" in L.vaqhip_last_error()
    v.mCodebook = codes[:100]
    v._ensure_codes()
    # bad arguments
    assert _kmeans(v, 101, seg)[0] == -1          # T > rows: the reference reads out of bounds
    assert _kmeans(v, 0, seg)[0] == -1
    assert _kmeans(v, T, 0)[0] == -1
    assert _kmeans(v, T, M + 1)[0] == -1
    assert _kmeans(v, T, seg, max_iter=0)[0] == -1
    assert L.vaqhip_index_cluster_ti_kmeans(None, T, seg, 50, None, None, None) == -1
    # the limits of set_ti_clusters
    assert _kmeans(v, 4097, seg)[0] == -2
    assert v.info()["ti_clusters"] == 0           # nothing was changed by the refused calls
    # the out-pointers may be NULL
    assert _kmeans(v, T, seg, want_out=False)[0] == 0
    assert v.info()["ti_clusters"] == T
    v.close()
    wide = VaqHip()                               # centres of more than 1024 dims
    wide.mBitsAlloc = [1] * 4
    wide.mCentroidsPerSubs = [np.zeros((2, 300), np.float32)] * 4
    wide.mCodebook = np.zeros((64, 4), np.uint16)
    wide._ensure_codes()
    assert _kmeans(wide, 2, 4)[0] == -2
    assert _kmeans(wide, 2, 3)[0] == 0            # 900 dims pass (all rows equal: one NaN centre, by the book)
    wide.close()


def test_refused_while_a_staged_search_is_open():
    import torch
    from vaq_amd import _lib
    from vaq_amd.index import VaqHip
    from helpers import make_case
    nq, k = 40, 50
    c = make_case(4508, 64, [8] * 8, 900_000, nq, dup_frac=0.02)
    v = VaqHip()
    v.mBitsAlloc = c["bits"]
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    v.set_option("bucket_major", 2)
    assert v.staged_supported(nq, k)
    Xd = torch.from_numpy(c["X"]).cuda()
    labels = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    dists = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    thr = torch.empty(nq, dtype=torch.int32, device="cuda")
    v.search_begin_device(Xd, k, (labels, dists), thr)
    assert _kmeans(v, 16, 2)[0] == -7
    assert b"staged" in _lib.load().vaqhip_last_error()
    v.search_finish_device(None)
    torch.cuda.synchronize()
    assert _kmeans(v, 16, 2, max_iter=2)[0] == 0
    v.close()


def test_again_and_after_add_codes():
    """A second call, and a call after add_codes, cluster the codes then present: the centres equal a fresh
    index's over the same rows (the second call starts from a TI-grouped index)."""
    name = "n4001_s5_l8_t24"
    N, seg, L, T, ncent, M = kr.CASES[name]
    codes, cents = kr.make_inputs(name)
    fx = kr.load_fixture(name)
    v = _index(name, codes[:3000])
    rc, first, _, _ = _kmeans(v, T, seg)
    assert rc == 0
    rc, again, _, _ = _kmeans(v, T, seg)
    assert rc == 0
    kr.assert_centres_equal(again, first, "second call")
    fresh = _index(name, codes[:3000])
    rc, want, _, _ = _kmeans(fresh, T, seg)
    assert rc == 0
    kr.assert_centres_equal(first, want, "fresh index over the first 3000 rows")
    fresh.close()
    v.add_codes(codes[3000:])
    rc, out, iters, nan_rows = _kmeans(v, T, seg)
    assert rc == 0
    kr.assert_centres_equal(out, fx["centres"], "after add_codes")
    assert (iters, nan_rows) == (int(fx["iterations"]), int(fx["nan_rows"].sum()))
    assert not np.array_equal(out.view(np.uint32), first.view(np.uint32))
    v.close()


# ---- the launch shapes of km_assign_kernel no fixture reaches ------------------------------------------------------
# Its row tile halves while R * d * 4 > 40960 bytes (d <= 40: 256 rows, 41..80: 128, 81..160: 64, wider: rows read
# from global memory) and its centres pass through LDS 4096 / d at a time.  The fixtures have d in {6, 12, 16, 20, 32,
# 40, 64, 512}: no case in 41..63 or 81..160, none at a boundary from above, and none on the global path with more
# than one turn of the staging loop.  name: (N, seg, L, T, centroids per subspace, subspaces of the index), as
# kmeans_ref.CASES; the expected centres are kmeans_ref.fit_codebook's, the restatement the fixtures pin.
TIER_CASES = {
    "d41": (321, 1, 41, 7, 64, 4),
    "d81": (321, 1, 81, 7, 64, 4),
    "d160": (321, 1, 160, 7, 64, 4),
    "d161": (321, 1, 161, 7, 64, 4),
    "d161_t30": (333, 1, 161, 30, 64, 4),
}


def _launch(d, T):
    """(rows per workgroup or "global", centres per stage) by the rules of kmeans_fit"""
    R = 256
    while R > 64 and R * d * 4 > 40 * 1024:
        R >>= 1
    return (R if R * d * 4 <= 40 * 1024 else "global"), max(1, min(T, 4096 // d))


def test_tier_cases_land_where_they_are_meant_to():
    got = {n: _launch(c[1] * c[2], c[3]) for n, c in TIER_CASES.items()}
    assert got == {"d41": (128, 7), "d81": (64, 7), "d160": (64, 7), "d161": ("global", 7), "d161_t30": ("global", 25)}
    for n, (N, seg, L, T, ncent, M) in TIER_CASES.items():
        R = got[n][0] if got[n][0] != "global" else 64
        assert N > R and N % R != 0 and N <= kr.ROWS_PER_CENTRE * T  # more than one workgroup, ragged, unsampled
    assert 30 * 161 > 4096 and 30 % 25 == 5  # two turns, the second clipped


@pytest.mark.parametrize("name", list(TIER_CASES))
def test_tile_tiers_equal_the_restatement(name):
    """Centres, iteration count and NaN rows bit for bit with kmeans_ref.fit on the decoded rows."""
    import hashlib
    from vaq_amd.index import VaqHip
    N, seg, L, T, ncent, M = TIER_CASES[name]
    rng = np.random.default_rng(int(hashlib.sha256(("tiers:" + name).encode()).hexdigest()[:8], 16))
    cents = [rng.normal(size=(ncent, L)).astype(np.float32) for _ in range(M)]
    codes = rng.integers(0, ncent, size=(N, M), dtype=np.int64).astype(np.uint16)
    want, want_iters, want_nan = kr.fit_codebook(codes, cents, seg, T)
    v = VaqHip()
    v.mBitsAlloc = [_bits(ncent)] * M
    v.mCentroidsPerSubs = cents
    v.mCodebook = codes
    v._ensure_codes()
    rc, out, iters, nan_rows = _kmeans(v, T, seg)
    v.close()
    assert rc == 0
    print(f"{name}: iterations {iters} (restatement {want_iters}), NaN centres {nan_rows} (restatement {int(want_nan.sum())})")
    kr.assert_centres_equal(out, want, name)
    assert iters == want_iters and iters >= 2
    assert nan_rows == int(want_nan.sum())
    assert np.array_equal(np.isnan(out).any(axis=1), want_nan)
