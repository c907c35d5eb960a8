"""Building a queryLUT index on the GPU: the quantile codebooks (vaqhip_lut_fit_quantiles) and the encoder
(vaqhip_encode_lut) of BitVecEngine::binaryEncodingLUT (BitVecEngine.hpp:811-840, :889-932), kernels in
vaq_amd/csrc/vaq_lutfit.hip.

Every comparison is plain equality against tests/lutfit_ref.py's numpy restatement -- centres and quantiles as
bit patterns, codes with array_equal; no tolerance.  The restatement itself is pinned against the host build of the
header the kernels run in tests/test_lutfit_cpu.py; neither is pinned against a compiled reference
(BitVecEngine.hpp needs glpk.h)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lutfit_ref as lr
import seq_exact_ref as sr

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def gpu_fit(vaqlib, X, bits, eig=None):
    """vaqhip_lut_fit_quantiles: (rc, centroidsMat 256 x D, Q D x 257); the outputs start as a pattern"""
    X = np.ascontiguousarray(X, np.float32)
    D = X.shape[1]
    cent = np.full((D, 256), 7.25, np.float32)
    q = np.full((D, 257), 7.25, np.float32)
    rc = vaqlib.vaqhip_lut_fit_quantiles(0, _p(X), X.shape[0], D, (C.c_int * D)(*bits), _p(eig), _p(cent), _p(q))
    return rc, np.ascontiguousarray(cent.T), q


def same_bits(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} differ, first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def ref_index(name):
    """a sequential-sum index over the restatement's centres and quantiles of a case"""
    import vaq_amd
    _, bits = lr.fit_case(name)
    cent, Qs = lr.fit_ref(name)
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = sr.centroid_list(bits, cent)
    v.mQuantiles = Qs
    return v


@pytest.mark.parametrize("name", lr.FIT_CASES)
def test_fit_matches_the_restatement(vaqlib, name):
    X, bits = lr.fit_case(name)
    rc, cent, Qs = gpu_fit(vaqlib, X, bits)
    assert rc == 0, vaqlib.vaqhip_last_error()
    want_c, want_q = lr.fit_ref(name)
    same_bits(Qs, want_q, f"{name} quantiles")
    same_bits(cent, want_c, f"{name} centres")


def test_fit_device_form_and_projection(vaqlib, oracle):
    """the _device form on a stream, and eigvec != NULL: the rows are projected first, unchecked"""
    import torch
    X, bits = lr.fit_case("n4099_d5")
    rng = np.random.default_rng(5)
    eig = np.linalg.qr(rng.normal(size=(5, 5)))[0].astype(np.float32)
    want_c, want_q = lr.fit(oracle.project(X, eig), bits)
    rc, cent, Qs = gpu_fit(vaqlib, X, bits, eig)
    assert rc == 0, vaqlib.vaqhip_last_error()
    same_bits(Qs, want_q, "projected quantiles")
    same_bits(cent, want_c, "projected centres")
    dx, de = torch.from_numpy(X).cuda(), torch.from_numpy(eig).cuda()
    dc = torch.empty((5, 256), dtype=torch.float32, device="cuda")
    dq = torch.empty((5, 257), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = vaqlib.vaqhip_lut_fit_quantiles_device(0, C.c_void_p(dx.data_ptr()), X.shape[0], 5, (C.c_int * 5)(*bits),
                                                C.c_void_p(de.data_ptr()), C.c_void_p(dc.data_ptr()),
                                                C.c_void_p(dq.data_ptr()), C.c_void_p(st))
    assert rc == 0, vaqlib.vaqhip_last_error()
    same_bits(dq.cpu().numpy(), want_q, "device form quantiles")
    same_bits(np.ascontiguousarray(dc.cpu().numpy().T), want_c, "device form centres")


def test_nan_in_the_training_rows_is_refused(vaqlib):
    """VAQHIP_EINVAL, the outputs untouched, and an index made before stays usable"""
    v = ref_index("n4099_d5")
    X, bits = lr.fit_case("n4099_d5")
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[4098, 3] = bad
        rc, cent, Qs = gpu_fit(vaqlib, Xb, bits)
        assert rc == -1 and b"NaN or infinite" in vaqlib.vaqhip_last_error()
        assert np.all(cent == 7.25) and np.all(Qs == 7.25)
    v.encodeLUT(lr.probes("n4099_d5"))
    assert np.array_equal(v.mCodebook, lr.codes_ref("n4099_d5"))
    rc, cent, Qs = gpu_fit(vaqlib, X, bits)
    assert rc == 0
    same_bits(cent, lr.fit_ref("n4099_d5")[0], "the fit after the refusals")
    v.close()


@pytest.mark.parametrize("name", lr.FIT_CASES)
def test_encode_matches_the_restatement(vaqlib, name):
    """Probes: every Q[q] itself and its two neighbours, the value midway between neighbouring centres, values
    below Q[0] and above Q[N], NaN, +-inf, training rows.  Host and _device forms."""
    import torch
    v = ref_index(name)
    P, want = lr.probes(name), lr.codes_ref(name)
    assert np.isnan(P).any() and np.isinf(P).any()
    v.encodeLUT(P)
    assert v.mCodebook.dtype == np.uint16
    bad = np.argwhere(v.mCodebook != want)
    assert bad.size == 0, f"{name}: probe {P[tuple(bad[0])]!r} (dim {bad[0][1]}) -> {v.mCodebook[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    d = v.encodeLUT_device(torch.from_numpy(P).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint16), want)
    v.close()


def test_encode_many_dimensions_in_tiles(vaqlib):
    """31 dimensions of 8 bits and one of 1 (an index packs at most 256 code bits): the tables exceed what a
    workgroup stages, so the encoder works in two tiles of dimensions; more rows than one chunk of a workgroup"""
    rng = np.random.default_rng(11)
    D, n = 32, 1500
    X = (rng.normal(size=(n, D)) * rng.uniform(0.5, 30, size=D)).astype(np.float32)
    bits = [8] * 31 + [1]
    rc, cent, Qs = gpu_fit(vaqlib, X, bits)
    assert rc == 0, vaqlib.vaqhip_last_error()
    import vaq_amd
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = sr.centroid_list(bits, cent)
    v.mQuantiles = Qs
    v.encodeLUT(X)
    assert np.array_equal(v.mCodebook, lr.encode(X, bits, cent, Qs))
    v.close()


def test_encode_projected_0_and_1(vaqlib, oracle):
    """projected = 0 applies the rotation first, unchecked (:620): a row with a NaN stays NaN in every
    coordinate and gets code N - 1 everywhere, where the query side's checked projection would make it 0"""
    import vaq_amd
    X, bits = lr.fit_case("n4099_d5")
    rng = np.random.default_rng(5)
    eig = np.linalg.qr(rng.normal(size=(5, 5)))[0].astype(np.float32)
    Xp = oracle.project(X, eig)
    cent, Qs = lr.fit(Xp, bits)
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(bits)
    v.mEigenVectors = eig
    v.mCentroidsPerSubs = sr.centroid_list(bits, cent)
    v.mQuantiles = Qs
    raw = X[:1000].copy()
    raw[7, 2] = np.nan
    want = lr.encode(oracle.project(raw, eig), bits, cent, Qs)
    assert np.all(want[7] == [(1 << b) - 1 for b in bits])
    v.encodeLUT(raw, projected=False)
    assert np.array_equal(v.mCodebook, want)
    v.encodeLUT(Xp[:1000], projected=True)
    assert np.array_equal(v.mCodebook, lr.encode(Xp[:1000], bits, cent, Qs))
    v.close()


def test_state_and_index_kind(vaqlib):
    import vaq_amd
    X, bits = lr.fit_case("n4099_d5")
    cent, Qs = lr.fit_ref("n4099_d5")
    codes = np.zeros((4, 5), np.uint16)
    v = ref_index("n4099_d5")
    v._ensure_index()
    assert vaqlib.vaqhip_encode_lut(v._h, _p(X), 4, 1, _p(codes)) == -7   # before the quantiles are set
    v.close()
    plain = vaq_amd.VaqHip()
    plain.mBitsAlloc = [8] * 4
    plain.mCentroidsPerSubs = [np.zeros((256, 1), np.float32)] * 4
    plain._ensure_index()
    assert vaqlib.vaqhip_index_set_lut_quantiles(plain._h, _p(np.zeros((4, 257), np.float32))) == -1
    plain.close()


@functools.lru_cache(maxsize=None)
def grid_queries():
    return np.random.default_rng(3).integers(-4, 5, size=(21, 4)).astype(np.float32)


def ref_answers(name, queries, k):
    _, bits = lr.fit_case(name)
    cent, Qs = lr.fit_ref(name)
    codes = lr.encode(lr.fit_case(name)[0], bits, cent, Qs)
    out = [sr.query_lut_topk(sr.row_dists(q, bits, cent, codes), k) for q in queries]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def test_end_to_end_build_and_exact_search(vaqlib):
    """fit -> create_ex(SEQUENTIAL) -> set_lut_quantiles -> encode_lut_device -> set_codes_u16_device -> search
    with exact_ties: the answer of seq_exact_ref over the restatement's centres and codes, slot for slot.  The
    integer grid: nearly every row ties with others."""
    import torch
    import vaq_amd
    X, bits = lr.fit_case("grid")
    k = 10
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(bits)
    v.fitQuantiles(X)
    same_bits(v.centroidsMat, lr.fit_ref("grid")[0], "fitQuantiles")
    codes = v.encodeLUT_device(torch.from_numpy(X).cuda())
    v.mCodebook = codes  # a device tensor: vaqhip_index_set_codes_u16_device
    v.set_option("exact_ties", 1)
    ans = v.search(grid_queries(), k)
    want_l, want_d = ref_answers("grid", grid_queries(), k)
    assert np.array_equal(ans.distances.reshape(-1, k).view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(ans.labels.reshape(-1, k), want_l)
    # the tie order matters here: the smallest-label rule gives other labels
    plain = [sr.smallest_label_topk(sr.row_dists(q, bits, lr.fit_ref("grid")[0], lr.encode(X, bits, *lr.fit_ref("grid"))), k)[0]
             for q in grid_queries()]
    assert not np.array_equal(np.stack(plain), want_l)
    v.close()


def test_demo_driver_builds_and_queries(vaqlib, tmp_path):
    """examples/demo_vaqhip.cpp --lut-bits: BitVecEngineHip::binaryEncodingLUT + queryLUT over a dataset file"""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    X, bits = lr.fit_case("grid")
    k = 10
    io.write_vecs(str(tmp_path / "base.fvecs"), X)
    io.write_vecs(str(tmp_path / "q.fvecs"), grid_queries())
    r = subprocess.run([exe, "--lut-bits", ",".join(map(str, bits)), "--dataset", str(tmp_path / "base.fvecs"),
                        "--queries", str(tmp_path / "q.fvecs"), "--timeseries-size", "4", "--k", str(k),
                        "--exact-ties", "1", "--result", str(tmp_path / "out.csv"), "--save-enc", str(tmp_path / "cb.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Encoding time" in r.stdout
    got = np.loadtxt(str(tmp_path / "out.csv"), delimiter=",", dtype=np.int64)
    assert np.array_equal(got, ref_answers("grid", grid_queries(), k)[0].astype(np.int64))
    assert np.array_equal(io.load_codebook(str(tmp_path / "cb.bin")), lr.encode(X, bits, *lr.fit_ref("grid")))
