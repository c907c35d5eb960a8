"""The subspace codebooks on the GPU (vaqhip_fit_codebooks*; vaq_amd/csrc/vaq_codebooks.hip): KMeans::staticFitSampling
per subspace, all subspaces per launch, against the centres recorded from the reference itself
(tests/golden/codebooks/README.md).  Every comparison is on bit patterns (NaN by position)."""
import ctypes as C
import functools

import numpy as np
import pytest

import codebooks_ref as cr
from helpers import assert_topk_matches

pytestmark = pytest.mark.gpu

PATTERN = np.float32(7.25)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@functools.lru_cache(maxsize=None)
def inputs(name):
    return cr.make_inputs(name)


def sizes(D, M, bits):
    L = D // M
    ks = [1 << b for b in bits]
    return L, ks, np.concatenate([[0], np.cumsum(ks)]) * L


def out_arrays(D, M, bits):
    """(centres, iterations, nan rows), preset to patterns a refusal must leave"""
    L, ks, offs = sizes(D, M, bits)
    return np.full(int(offs[-1]), PATTERN, np.float32), np.full(M, -9, np.int32), np.full(M, -9, np.int32)


def split(cent, D, M, bits):
    L, ks, offs = sizes(D, M, bits)
    return [cent[offs[s]:offs[s + 1]].reshape(ks[s], L) for s in range(M)]


def host_fit(L_, X, M, bits, eig=None, max_iter=cr.MAX_ITER, fn=None):
    """vaqhip_fit_codebooks (or its _u8 twin): (rc, [M centre matrices], iterations, nan rows)"""
    n, D = X.shape
    cent, iters, nan = out_arrays(D, M, bits)
    fn = fn or (L_.vaqhip_fit_codebooks_u8 if X.dtype == np.uint8 else L_.vaqhip_fit_codebooks)
    rc = fn(0, _p(X), n, D, M, (C.c_int * M)(*bits), _p(eig), max_iter, _p(cent), _p(iters), _p(nan))
    return rc, split(cent, D, M, bits), iters, nan


def device_fit(L_, d_X, n, D, M, bits, eig=None, max_iter=cr.MAX_ITER):
    """the _device forms on a torch tensor (float32 or uint8, any byte address)"""
    import torch
    L, ks, offs = sizes(D, M, bits)
    d_cent = torch.full((int(offs[-1]),), float(PATTERN), dtype=torch.float32, device="cuda")
    d_eig = torch.from_numpy(eig).cuda() if eig is not None else None
    iters, nan = np.full(M, -9, np.int32), np.full(M, -9, np.int32)
    fn = L_.vaqhip_fit_codebooks_u8_device if d_X.dtype == torch.uint8 else L_.vaqhip_fit_codebooks_device
    torch.cuda.synchronize()
    rc = fn(0, C.c_void_p(d_X.data_ptr()), n, D, M, (C.c_int * M)(*bits),
            C.c_void_p(d_eig.data_ptr()) if d_eig is not None else None, max_iter, C.c_void_p(d_cent.data_ptr()),
            _p(iters), _p(nan), None)
    return rc, split(d_cent.cpu().numpy(), D, M, bits), iters, nan


def same_fit(got, want, what):
    assert got[0] == 0, what
    for s, (g, w) in enumerate(zip(got[1], want[1])):
        cr.assert_centres_equal(g, w, f"{what}, subspace {s}")
    assert np.array_equal(got[2], want[2]), f"{what}: iterations {got[2]} vs {want[2]}"
    assert np.array_equal(got[3], want[3]), f"{what}: NaN rows {got[3]} vs {want[3]}"


@functools.lru_cache(maxsize=None)
def fitted(name):
    """the host form's answer for a fixture case, computed once"""
    from vaq_amd import _lib
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = inputs(name)
    return host_fit(_lib.load(), X, M, bits, eig)


@pytest.mark.parametrize("name", list(cr.CASES))
def test_fixtures_through_the_host_form(vaqlib, name):
    """Every recorded case: centres, the reference's iter_count and the NaN centres per subspace."""
    n, D, M, bits, kind, salt = cr.CASES[name]
    fx = cr.load_fixture(name)
    rc, cents, iters, nan = fitted(name)
    assert rc == 0, vaqlib.vaqhip_last_error()
    for s in range(M):
        cr.assert_centres_equal(cents[s], fx["centres_%d" % s], f"{name}, subspace {s}")
        assert iters[s] == int(fx["iterations_%d" % s]), (name, s, iters)
        assert nan[s] == int(fx["nan_rows_%d" % s].sum()), (name, s, nan)
        assert np.array_equal(np.isnan(cents[s]).any(axis=1), fx["nan_rows_%d" % s])


def test_forms_agree_on_float_rows(vaqlib):
    """`sampled` (the host form gathers its sample on the host, the others on the device) and `mixed` (one subspace
    reads all rows in place, the device gathers the others' sample in every form): the _device form and the refiner
    over float rows equal the host form."""
    import torch
    import vaq_amd
    for name in ("sampled", "mixed"):
        n, D, M, bits, kind, salt = cr.CASES[name]
        X, _ = inputs(name)
        want = fitted(name)
        same_fit(device_fit(vaqlib, torch.from_numpy(X).cuda(), n, D, M, bits), want, name + " _device")
        r = vaq_amd.VaqRefiner(D)
        r.set_rows(X)
        cents, iters, nan = r.fit_codebooks(M, bits)
        same_fit((0, cents, iters, nan), want, name + " refiner, float rows")
        r.close()


def test_forms_agree_on_byte_rows(vaqlib):
    """`bytes`, a byte matrix large enough to be sampled, one of `mixed`'s shape (values 0..255: all rows widened
    for the subspace that does not sample, the sample gathered from them) and `dupes` (two turns of the centre staging
    loop): _u8 and _u8_device equal the float form on the widened matrix; a byte pointer at an odd offset gives the
    aligned result; so does the refiner over byte rows."""
    import torch
    import vaq_amd
    big = np.random.default_rng(77).integers(0, 256, size=(66001, 8), dtype=np.int64).astype(np.uint8)
    n, D, M, bits, kind, salt = cr.CASES["mixed"]
    mixed = np.random.default_rng(78).integers(0, 256, size=(n, D), dtype=np.int64).astype(np.uint8)
    for what, X8, M, bits in (("bytes", inputs("bytes")[0], 4, cr.CASES["bytes"][3]), ("sampled bytes", big, 2, (3, 2)),
                              ("mixed bytes", mixed, M, bits), ("dupes", inputs("dupes")[0], 1, cr.CASES["dupes"][3])):
        n, D = X8.shape
        want = host_fit(vaqlib, X8.astype(np.float32), M, bits)
        assert want[0] == 0
        same_fit(host_fit(vaqlib, X8, M, bits), want, what + " _u8")
        same_fit(device_fit(vaqlib, torch.from_numpy(X8).cuda(), n, D, M, bits), want, what + " _u8_device")
        buf = torch.zeros(n * D + 3, dtype=torch.uint8, device="cuda")
        odd = buf[3:3 + n * D].view(n, D)
        odd.copy_(torch.from_numpy(X8))
        assert odd.data_ptr() % 4 == 3
        same_fit(device_fit(vaqlib, odd, n, D, M, bits), want, what + " _u8_device at an odd address")
        r = vaq_amd.VaqRefiner(D)
        r.set_rows_u8(X8)
        cents, iters, nan = r.fit_codebooks(M, bits)
        same_fit((0, cents, iters, nan), want, what + " refiner, byte rows")
        r.close()
    cents, iters, nan = vaq_amd.fit_codebooks_u8(inputs("bytes")[0], 4, cr.CASES["bytes"][3])
    same_fit((0, cents, iters, nan), fitted("bytes"), "vaq_amd.fit_codebooks_u8")


def rotated_index(cents):
    import vaq_amd
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = [np.ascontiguousarray(c) for c in cents]
    v.mEigenVectors = inputs("rotated")[1]
    return v


def test_rotation_in_front_is_the_projection(vaqlib):
    """`rotated`: fitting with eigvec equals fitting, with eigvec = NULL, the matrix vaqhip_project returns."""
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = inputs("rotated")
    want = fitted("rotated")
    v = rotated_index(want[1])
    P = v.project(X)
    v.close()
    assert not np.array_equal(P, X)
    same_fit(host_fit(vaqlib, P, M, bits, None), want, "fit of the projected matrix")


def test_rotation_in_front_of_a_mixed_batch(vaqlib):
    """`mixed` behind a random orthogonal eigvec (all rows are projected once and the sample is gathered from the
    projected matrix): the fit equals the fit, with eigvec = NULL, of the matrix vaqhip_project returns."""
    import vaq_amd
    n, D, M, bits, kind, salt = cr.CASES["mixed"]
    X, _ = inputs("mixed")
    q, _ = np.linalg.qr(np.random.default_rng(79).normal(size=(D, D)))
    eig = np.ascontiguousarray(q, np.float32)
    v = vaq_amd.VaqHip(sequential_sum=True)  # any index of D columns projects: one 1-bit quantiser per column
    v.mBitsAlloc = [1] * D
    v.mCentroidsPerSubs = [np.array([[0.0], [1.0]], np.float32) for _ in range(D)]
    v.mEigenVectors = eig
    P = v.project(X)
    v.close()
    assert not np.array_equal(P, X)
    want = host_fit(vaqlib, P, M, bits, None)
    assert want[0] == 0, vaqlib.vaqhip_last_error()
    same_fit(host_fit(vaqlib, X, M, bits, eig), want, "mixed, eigvec in front")
    assert not np.array_equal(want[1][0], fitted("mixed")[1][0])


@pytest.mark.parametrize("name", ["tiny", "prefix", "mixed"])
def test_batching_changes_nothing(vaqlib, name):
    """Subspace s alone (M = 1 on its column block, copied dense) equals subspace s of the batched call: the
    reference's own calling pattern, every call sampling for itself."""
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, _ = inputs(name)
    L = D // M
    want = fitted(name)
    for s in range(M):
        rc, cents, iters, nan = host_fit(vaqlib, np.ascontiguousarray(X[:, s * L:(s + 1) * L]), 1, [bits[s]])
        assert rc == 0
        cr.assert_centres_equal(cents[0], want[1][s], f"{name}, subspace {s} alone")
        assert iters[0] == want[2][s] and nan[0] == want[3][s]


def test_repeatable_and_undisturbed(vaqlib):
    """Twice the same; a call with other shapes in between on the same thread changes nothing."""
    import vaq_amd
    for name in ("odd", "wide", "odd", "bytes", "tiny", "odd"):
        n, D, M, bits, kind, salt = cr.CASES[name]
        X, eig = inputs(name)
        same_fit(host_fit(vaqlib, X, M, bits, eig), fitted(name), name + " again")
    cents, iters, nan = vaq_amd.fit_codebooks(inputs("odd")[0], 2, cr.CASES["odd"][3])
    same_fit((0, cents, iters, nan), fitted("odd"), "vaq_amd.fit_codebooks")
    t = vaq_amd.last_fit_codebooks_timing()
    assert t["sample_rows"] == 4001 and t["iterations"] == max(fitted("odd")[2]) and t["subspaces"] == 2
    # sample_rows: the most rows a subspace works on -- all of them as soon as one subspace does not sample
    for name, rows in (("sampled", 65536), ("mixed", 66000)):
        n, D, M, bits, kind, salt = cr.CASES[name]
        same_fit(host_fit(vaqlib, inputs(name)[0], M, bits), fitted(name), name + " again")
        t = vaq_amd.last_fit_codebooks_timing()
        assert t["sample_rows"] == rows and t["rows"] == n and t["subspaces"] == M


def test_max_iter_and_late_refusal_leave_outputs(vaqlib):
    """max_iter cuts every subspace; a row without any centre in reach (an infinite value) is refused after the run
    and the outputs keep their contents."""
    n, D, M, bits, kind, salt = cr.CASES["odd"]
    X, _ = inputs("odd")
    rc, cents, iters, nan = host_fit(vaqlib, X, M, bits, max_iter=2)
    assert rc == 0 and list(iters) == [2, 2]
    want, it = cr.fit(np.ascontiguousarray(X[:, :D // M]), 1 << bits[0], 2)
    cr.assert_centres_equal(cents[0], want, "two iterations")
    bad = X.copy()
    bad[:, 0] = np.inf  # every distance of subspace 0 is inf or NaN
    rc, cents, iters, nan = host_fit(vaqlib, bad, M, bits)
    assert rc == -1 and b"row -1" in vaqlib.vaqhip_last_error()
    assert all(np.all(c == PATTERN) for c in cents) and np.all(iters == -9) and np.all(nan == -9)


def test_end_to_end_fit_create_encode_search(vaqlib, oracle):
    """`rotated`: fit, vaqhip_index_create, vaqhip_encode, set_codes, search -- the search is oracle.search's over
    those centroids and codes, and Lloyd's property holds: the mean squared distance of the sample rows to their
    nearest centre is lower with the fitted centres than with the seeds, in every subspace."""
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = inputs("rotated")
    rc, cents, iters, nan = fitted("rotated")
    assert rc == 0 and not nan.any()
    v = rotated_index(cents)
    v.encode(X, projected=False)
    codes = v.mCodebook
    k, Q = 10, X[:37] + np.float32(0.125)
    ans = v.search(Q, k)
    v.close()
    o_lab, o_dis = oracle.search(Q, [np.ascontiguousarray(c) for c in cents], codes, k, eig=eig)
    assert_topk_matches(ans.labels.reshape(-1, k), ans.distances.reshape(-1, k), o_lab, o_dis, what="fitted index")
    P = cr.projected_sample(X, eig, bits).astype(np.float64)
    L = D // M
    for s in range(M):
        Ps = P[:, s * L:(s + 1) * L]
        seeds = Ps[cr.permutation_head(n, 1 << bits[s])]

        def cost(c):
            return ((Ps[:, None, :] - c[None, :, :]) ** 2).sum(-1).min(1).mean()
        assert cost(cents[s].astype(np.float64)) < cost(seeds), s
        # and the codes are the nearest fitted centre's
        assert codes[:, s].max() < (1 << bits[s])


def test_demo_fits_and_saves(vaqlib, tmp_path):
    """demo_vaqhip --fit-codebooks ... --save, then loadCentroids' format read back, equals the Python call's centres
    (the C++ adapter path); from the fvecs file, and from the resident rows."""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = inputs("rotated")
    io.write_vecs(str(tmp_path / "base.fvecs"), X)
    eig.tofile(str(tmp_path / "eig.f32"))
    want = fitted("rotated")
    for extra in ([], ["--refine-resident"]):
        out = tmp_path / ("c%d.bin" % len(extra))
        r = subprocess.run([exe, "--fit-codebooks", "--bits", ",".join(map(str, bits)), "--dataset", str(tmp_path / "base.fvecs"),
                            "--eigen", str(tmp_path / "eig.f32"), "--timeseries-size", str(D), "--save", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Codebook fit time" in r.stdout and "iterations " + " ".join(map(str, want[2])) in r.stdout
        got = io.load_centroids(str(out))
        assert len(got) == M
        for s in range(M):
            cr.assert_centres_equal(got[s], want[1][s], f"demo {extra}, subspace {s}")
    # ... and composed with --encode: the whole index from the raw vectors, queried
    k, Q = 5, X[:9] + np.float32(0.125)
    io.write_vecs(str(tmp_path / "q.fvecs"), Q)
    r = subprocess.run([exe, "--fit-codebooks", "--encode", "--bits", ",".join(map(str, bits)), "--dataset", str(tmp_path / "base.fvecs"),
                        "--eigen", str(tmp_path / "eig.f32"), "--timeseries-size", str(D), "--queries", str(tmp_path / "q.fvecs"),
                        "--k", str(k), "--save-enc", str(tmp_path / "cb.bin"), "--result", str(tmp_path / "out.csv")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    v = rotated_index(want[1])
    v.encode(X, projected=False)
    assert np.array_equal(io.load_codebook(str(tmp_path / "cb.bin")), v.mCodebook)
    labels = v.search(Q, k).labels.reshape(-1, k)
    v.close()
    assert np.array_equal(np.loadtxt(str(tmp_path / "out.csv"), delimiter=",", dtype=np.int64), labels.astype(np.int64))
