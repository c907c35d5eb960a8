"""The CPU side of building a queryLUT index on the GPU (BitVecEngine::binaryEncodingLUT from the bit
allocation on): the C ABI is there, refuses what it must without a device, the numpy restatement
(tests/lutfit_ref.py) has the properties the reference's code implies, and the header the kernels run
(vaq_amd/csrc/vaq_lutfit.h), built for the host, agrees with it bit for bit (tests/cpp/lutfit_test.cpp, once
more under AddressSanitizer + UBSan: host code only, its own main)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lutfit_ref as lr

NEW_SYMBOLS = ("vaqhip_lut_fit_quantiles", "vaqhip_lut_fit_quantiles_device", "vaqhip_index_set_lut_quantiles",
               "vaqhip_encode_lut", "vaqhip_encode_lut_device", "vaqhip_lut_fit_set_timing",
               "vaqhip_last_lut_fit_timing")


def test_symbols_and_version(vaqlib):
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 110
    for s in NEW_SYMBOLS:
        assert hasattr(vaqlib, s) and s in _lib.SYMBOLS, s
    import vaq_amd
    for m in ("fitQuantiles", "encodeLUT", "encodeLUT_device"):
        assert hasattr(vaq_amd.VaqHip, m), m


def test_refusals_that_need_no_device(vaqlib):
    X = np.zeros((4, 2), np.float32)
    cent = np.zeros((2, 256), np.float32)
    q = np.zeros((2, 257), np.float32)

    def fit(n, D, bits, x=X, c=cent, qq=q):
        b = (C.c_int * len(bits))(*bits) if bits is not None else None
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        return vaqlib.vaqhip_lut_fit_quantiles(0, p(x), n, D, b, None, p(c), p(qq))

    assert fit(4, 2, [0, 3]) == -1 and b"bits[0]=0" in vaqlib.vaqhip_last_error()
    assert fit(4, 2, [3, 9]) == -1 and b"bits[1]=9" in vaqlib.vaqhip_last_error()
    assert fit(0, 2, [3, 3]) == -1
    assert fit(-5, 2, [3, 3]) == -1
    assert fit(1 << 31, 2, [3, 3]) == -1
    assert fit(4, 0, []) == -1
    assert fit(4, 2, None) == -1
    assert fit(4, 2, [3, 3], x=None) == -1
    assert fit(4, 2, [3, 3], c=None) == -1
    assert fit(4, 2, [3, 3], qq=None) == -1
    assert vaqlib.vaqhip_lut_fit_quantiles_device(0, None, 4, 2, (C.c_int * 2)(3, 3), None, None, None, None) == -1
    assert vaqlib.vaqhip_index_set_lut_quantiles(None, q.ctypes.data_as(C.c_void_p)) == -1
    assert vaqlib.vaqhip_encode_lut(None, None, 1, 1, None) == -1
    assert vaqlib.vaqhip_encode_lut_device(None, None, 1, 1, None, None) == -1
    assert vaqlib.vaqhip_last_lut_fit_timing(None) == -1


def test_python_adapter_is_for_sequential_sum_indexes():
    import vaq_amd
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = [3, 3]
    with pytest.raises(vaq_amd.VaqHipError) as e:
        v.fitQuantiles(np.zeros((4, 2), np.float32))
    assert e.value.code == -1
    with pytest.raises(vaq_amd.VaqHipError) as e:
        v.encodeLUT(np.zeros((4, 2), np.float32))
    assert e.value.code == -1
    s = vaq_amd.VaqHip(sequential_sum=True)
    s.mBitsAlloc = [3, 3]
    with pytest.raises(vaq_amd.VaqHipError) as e:
        s.encodeLUT(np.zeros((4, 2), np.float32))
    assert e.value.code == -7  # no quantiles yet


# ---- properties of the restatement ----
@pytest.mark.parametrize("name", lr.FIT_CASES)
def test_quantile_ends_and_centres(name):
    X, bits = lr.fit_case(name)
    cent, Qs = lr.fit_ref(name)
    assert cent.shape == (256, X.shape[1]) and Qs.shape == (X.shape[1], 257)
    for d, b in enumerate(bits):
        N = 1 << b
        assert Qs[d, 0] == X[:, d].min() and Qs[d, N] == X[:, d].max()
        assert np.all(Qs[d, N + 1:] == 0) and np.all(cent[N:, d] == 0)
        assert np.all(np.isfinite(Qs[d])) and np.all(np.isfinite(cent[:, d]))
        # a centre is a mean of training values or a midpoint of two quantiles: inside the column's range, up
        # to the rounding of n sequential float32 adds (n * 2^-24 relative; a constant column shows it)
        slack = np.float64(X.shape[0]) * 2.0 ** -24 * np.abs(X[:, d]).max()
        assert np.all(cent[:N, d] >= X[:, d].min() - slack) and np.all(cent[:N, d] <= X[:, d].max() + slack)


@pytest.mark.parametrize("name", lr.FIT_CASES)
def test_chosen_code_is_a_nearest_centre_of_its_candidates(name):
    """Inside the training range the chosen code is a nearest centre of ALL centres, and equals vaqhip_encode's
    first argmin whenever that minimum is attained once -- in every column whose centres ascend and lie in their
    own buckets, Q[i] <= c[i] <= Q[i+1]: the up to three candidates then bracket the row.  (Not so in a
    degenerate column: all rows equal, the rounded mean of a bucket can leave it by an ulp and the reference
    still answers code 0 for x == Q[0]; those columns only go through the out-of-range checks below.)"""
    X, bits = lr.fit_case(name)
    cent, Qs = lr.fit_ref(name)
    P = lr.probes(name)
    codes = lr.codes_ref(name)
    assert codes.dtype == np.uint16 and codes.shape == P.shape
    checked_argmin = 0
    for d, b in enumerate(bits):
        N = 1 << b
        c = cent[:N, d]
        x = P[:, d]
        code = codes[:, d].astype(np.int64)
        assert np.all(code < N)
        fin = np.isfinite(x) & (x >= Qs[d, 0]) & (x <= Qs[d, N])  # inside the training range
        with np.errstate(invalid="ignore", over="ignore"):
            dist = np.abs((x[:, None] - c[None, :]).astype(np.float32))
        chosen = dist[np.arange(x.size), code]
        if np.all(np.diff(c) >= 0) and np.all(c >= Qs[d, :N]) and np.all(c <= Qs[d, 1:N + 1]):
            assert np.all(chosen[fin] == dist[fin].min(axis=1)), (name, d)
            distinct = fin & ((dist == dist.min(axis=1, keepdims=True)).sum(axis=1) == 1)
            assert np.array_equal(code[distinct], lr.first_argmin(x, c, N)[distinct]), (name, d)
            checked_argmin += int(distinct.sum())
        # outside the range and NaN: the reference's own answers
        assert np.all(code[np.isnan(x)] == N - 1)
        assert np.all(code[x == -np.inf] == 0)
        assert np.all(code[x > Qs[d, :N + 1].max()] == N - 1)
        assert np.all(code[x < Qs[d, 0]] == 0)
    if name not in ("const", "n1"):
        assert checked_argmin > 100


def test_ties_differ_from_the_first_argmin():
    """Where vaqhip_encode cannot stand in: on the integer grid some probe lies exactly midway between two
    centres and the engine's <= preference takes the bucket's own centre, not the first argmin."""
    X, bits = lr.fit_case("grid")
    cent, Qs = lr.fit_ref("grid")
    P, codes = lr.probes("grid"), lr.codes_ref("grid")
    differ = 0
    for d, b in enumerate(bits):
        N = 1 << b
        fin = np.isfinite(P[:, d])
        differ += int((codes[fin, d] != lr.first_argmin(P[:, d], cent[:N, d], N)[fin]).sum())
    assert differ > 0


def test_sequential_sum_is_not_a_pairwise_sum():
    """The contract is the order of the adds: a case where numpy's pairwise float32 sum gives another centre."""
    X, bits = lr.fit_case("n70001_b1")
    Z = lr.sort_column(X[:, 0])
    Q, c = lr.centroids_quantile(Z, 2)
    end = int(np.searchsorted(Z, Q[1], side="right"))
    pair = np.float32(Z[:end].sum(dtype=np.float32)) / np.float32(end)
    seq = np.float32(0)
    for v in Z[:end]:
        seq = np.float32(seq + v)
    assert c[0] == np.float32(seq) / np.float32(end)
    assert c[0] != pair


# ---- the header the kernels run, built for the host ----
def test_shared_header_matches_the_restatement(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        np.array([len(lr.FIT_CASES)], np.int32).tofile(f)
        for name in lr.FIT_CASES:
            X, bits = lr.fit_case(name)
            cent, Qs = lr.fit_ref(name)
            P, codes = lr.probes(name), lr.codes_ref(name)
            np.array([X.shape[0], X.shape[1], P.shape[0]], np.int32).tofile(f)
            np.array(bits, np.int32).tofile(f)
            np.ascontiguousarray(X).tofile(f)
            np.ascontiguousarray(P).tofile(f)
            np.ascontiguousarray(cent.T).tofile(f)  # [D][256]
            np.ascontiguousarray(Qs).tofile(f)
            np.ascontiguousarray(codes).tofile(f)
    for extra, name in ((["-O2"], "lutfit_test"),
                        (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "lutfit_asan")):
        exe = str(tmp_path / name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [os.path.join(root, "tests", "cpp", "lutfit_test.cpp"), "-o", exe])
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert f"lutfit_test: ok ({len(lr.FIT_CASES)} cases)" in r.stdout
