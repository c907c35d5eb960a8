"""The hierarchical codebook fit on the GPU (vaqhip_fit_codebooks_hier*; vaq_amd/csrc/vaq_codebooks.hip): subspaces
above 8 bits as 128 centres, a split of the rows by nearest centre and 1 << (bits - 7) centres per group, against the
composition of the pinned numpy restatements (tests/codebooks_hier_ref.py).  Every comparison is on bit patterns (NaN
by position), plus the iteration counts and the NaN centres per subspace."""
import ctypes as C
import functools

import numpy as np
import pytest

import codebooks_hier_ref as hr
import codebooks_ref as cr
from helpers import assert_topk_matches
from test_codebooks_gpu import PATTERN, _p, host_fit as flat_host_fit, same_fit, split

pytestmark = pytest.mark.gpu


def hier_fit(L_, X, M, bits, eig=None, max_iter=cr.MAX_ITER):
    """vaqhip_fit_codebooks_hier (or its _u8 twin): (rc, [M centre matrices], iterations, nan rows)"""
    return flat_host_fit(L_, X, M, bits, eig, max_iter,
                         fn=L_.vaqhip_fit_codebooks_hier_u8 if X.dtype == np.uint8 else L_.vaqhip_fit_codebooks_hier)


def hier_device_fit(L_, d_X, n, D, M, bits, eig=None, max_iter=cr.MAX_ITER):
    import torch
    ks = [1 << b for b in bits]
    d_cent = torch.full((sum(ks) * (D // M),), float(PATTERN), dtype=torch.float32, device="cuda")
    d_eig = torch.from_numpy(eig).cuda() if eig is not None else None
    iters, nan = np.full(M, -9, np.int32), np.full(M, -9, np.int32)
    fn = L_.vaqhip_fit_codebooks_hier_u8_device if d_X.dtype == torch.uint8 else L_.vaqhip_fit_codebooks_hier_device
    torch.cuda.synchronize()
    rc = fn(0, C.c_void_p(d_X.data_ptr()), n, D, M, (C.c_int * M)(*bits),
            C.c_void_p(d_eig.data_ptr()) if d_eig is not None else None, max_iter, C.c_void_p(d_cent.data_ptr()),
            _p(iters), _p(nan), None)
    return rc, split(d_cent.cpu().numpy(), D, M, bits), iters, nan


def oracle_fit(name):
    """the oracle's answer in the shape of hier_fit's"""
    cents, iters, nans, info = hr.expected(name)
    return 0, cents, np.array(iters, np.int32), np.array([int(m.sum()) for m in nans], np.int32)


@functools.lru_cache(maxsize=None)
def fitted(name):
    """the host form's answer for a case, computed once"""
    from vaq_amd import _lib
    n, D, M, bits, kind, salt = hr.CASES[name]
    X, eig = hr.inputs(name)
    return hier_fit(_lib.load(), X, M, bits, eig)


@pytest.mark.parametrize("name", list(hr.CASES))
def test_cases_against_the_oracle(vaqlib, name):
    """Every case of the table: centres bit for bit, the largest iteration count of the 129 fits, the NaN centres."""
    got = fitted(name)
    assert got[0] == 0, vaqlib.vaqhip_last_error()
    same_fit(got, oracle_fit(name), name)


def test_flat_subspace_beside_a_hierarchical_one(vaqlib):
    """`tiny`: subspace 1 (3 bits) equals vaqhip_fit_codebooks's subspace 1; subspace 0 does not (it is hierarchical)."""
    n, D, M, bits, kind, salt = hr.CASES["tiny"]
    X, _ = hr.inputs("tiny")
    flat = flat_host_fit(vaqlib, X, M, bits)
    got = fitted("tiny")
    assert flat[0] == 0 and got[0] == 0
    cr.assert_centres_equal(got[1][1], flat[1][1], "flat subspace of tiny")
    assert got[2][1] == flat[2][1] and got[3][1] == flat[3][1]
    assert not np.array_equal(got[1][0], flat[1][0])


@pytest.mark.parametrize("name", ["bytes", "odd"])
def test_no_wide_subspace_is_the_flat_fit(vaqlib, name):
    """All bits <= 8: vaqhip_fit_codebooks's result bit for bit."""
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = cr.make_inputs(name)
    want = flat_host_fit(vaqlib, X, M, bits, eig)
    assert want[0] == 0
    same_fit(hier_fit(vaqlib, X, M, bits, eig), want, name + " through the hierarchical call")


def test_forms_agree_on_two(vaqlib):
    """`two` through the _device form, the refiner and the Python call; the timing names its 256 groups."""
    import torch
    import vaq_amd
    n, D, M, bits, kind, salt = hr.CASES["two"]
    X, eig = hr.inputs("two")
    want = fitted("two")
    assert want[0] == 0, vaqlib.vaqhip_last_error()
    same_fit(hier_device_fit(vaqlib, torch.from_numpy(X).cuda(), n, D, M, bits, eig), want, "two _device")
    r = vaq_amd.VaqRefiner(D)
    r.set_rows(X)
    cents, iters, nan = r.fit_codebooks_hier(M, bits, eig)
    r.close()
    same_fit((0, cents, iters, nan), want, "two refiner")
    cents, iters, nan = vaq_amd.fit_codebooks_hier(X, M, bits, eig)
    same_fit((0, cents, iters, nan), want, "vaq_amd.fit_codebooks_hier")
    t = vaq_amd.last_fit_codebooks_hier_timing()
    info = hr.expected("two")[3]
    sizes = np.concatenate([info[s]["sizes"] for s in sorted(info)])
    assert t["groups"] == 256 and t["hier_subspaces"] == 2 and t["subspaces"] == M and t["rows"] == n
    assert (t["min_group_rows"], t["max_group_rows"]) == (sizes.min(), sizes.max())
    assert t["stage2_iterations"] == max(max(info[s]["it2"]) for s in info)


def test_byte_rows_are_the_widened_rows(vaqlib):
    """`two`'s shape as uint8 rows with values 0..255 behind its eigvec: _u8, _u8_device and the refiner over byte rows
    equal the float call on the widened rows, which equals the oracle."""
    import torch
    import vaq_amd
    n, D, M, bits, kind, salt = hr.CASES["two"]
    X8, eig = hr.byte_inputs()
    want = hier_fit(vaqlib, X8.astype(np.float32), M, bits, eig)
    assert want[0] == 0, vaqlib.vaqhip_last_error()
    cents, iters, nans, info = hr.expected_bytes()
    same_fit(want, (0, cents, np.array(iters, np.int32), np.array([int(m.sum()) for m in nans], np.int32)), "widened bytes")
    same_fit(hier_fit(vaqlib, X8, M, bits, eig), want, "two _u8")
    same_fit(hier_device_fit(vaqlib, torch.from_numpy(X8).cuda(), n, D, M, bits, eig), want, "two _u8_device")
    r = vaq_amd.VaqRefiner(D)
    r.set_rows_u8(X8)
    got = r.fit_codebooks_hier(M, bits, eig)
    r.close()
    same_fit((0,) + tuple(got), want, "two refiner, byte rows")
    got = vaq_amd.fit_codebooks_hier_u8(X8, M, bits, eig)
    same_fit((0,) + tuple(got), want, "vaq_amd.fit_codebooks_hier_u8")


def test_refusals_leave_the_outputs(vaqlib):
    """Fewer than 128 distinct slices under a 9-bit subspace: a stage-1 centre cannot be fitted -- EINVAL after stage 1,
    the message names the subspace, the outputs keep their contents.  rows_s < k_s: refused before any device work."""
    rng = np.random.default_rng(5)
    few = rng.normal(size=(100, 2)).astype(np.float32)
    X = np.ascontiguousarray(np.concatenate([rng.normal(size=(2000, 2)).astype(np.float32), few[rng.integers(0, 100, 2000)]], axis=1))
    rc, cents, iters, nan = hier_fit(vaqlib, X, 2, (3, 9))
    assert rc == -1, rc
    assert b"subspace 1" in vaqlib.vaqhip_last_error(), vaqlib.vaqhip_last_error()
    assert all(np.all(c == PATTERN) for c in cents) and np.all(iters == -9) and np.all(nan == -9)
    rc, cents, iters, nan = hier_fit(vaqlib, X[:300], 2, (3, 9))
    assert rc == -1 and b"out of bounds" in vaqlib.vaqhip_last_error()
    assert all(np.all(c == PATTERN) for c in cents) and np.all(iters == -9) and np.all(nan == -9)


def test_end_to_end_fit_create_encode_search(vaqlib, oracle):
    """`two`: the hierarchical centres go to vaqhip_index_create, vaqhip_encode and the search; labels and distances are
    oracle.search's over the same centres and codes."""
    import vaq_amd
    n, D, M, bits, kind, salt = hr.CASES["two"]
    X, eig = hr.inputs("two")
    rc, cents, iters, nan = fitted("two")
    assert rc == 0
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = [np.ascontiguousarray(c) for c in cents]
    v.mEigenVectors = eig
    v.encode(X, projected=False)
    codes = v.mCodebook
    assert codes[:, 0].max() >= 256  # (the wide subspace is used beyond a byte)
    k, Q = 10, X[:37] + np.float32(0.125)
    ans = v.search(Q, k)
    v.close()
    o_lab, o_dis = oracle.search(Q, [np.ascontiguousarray(c) for c in cents], codes, k, eig=eig)
    assert_topk_matches(ans.labels.reshape(-1, k), ans.distances.reshape(-1, k), o_lab, o_dis, what="hierarchical index")


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/fit_codebooks_hier_shim_test.cpp: VaqHip with mHierarchicalKmeans returns the C call's centres, with
    it clear today's; after setDevices() the flag is refused."""
    import os
    import subprocess
    from vaq_amd import build
    n, D, M, bits, kind, salt = hr.CASES["two"]
    X, eig = hr.inputs("two")
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([n, D, M], np.int32).tobytes())
        f.write(np.array(bits, np.int32).tobytes())
        f.write(eig.tobytes())
        f.write(X.tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fit_codebooks_hier_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "fit_codebooks_hier_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fit_codebooks_hier_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_kmeans_ver(vaqlib, tmp_path):
    """demo_vaqhip --fit-codebooks --kmeans-ver 1 --save: the saved centres are the hierarchical call's; --kmeans-ver 2
    is refused with a message."""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    n, D, M, bits, kind, salt = hr.CASES["two"]
    X, eig = hr.inputs("two")
    io.write_vecs(str(tmp_path / "base.fvecs"), X)
    eig.tofile(str(tmp_path / "eig.f32"))
    want = fitted("two")
    args = [exe, "--fit-codebooks", "--bits", ",".join(map(str, bits)), "--dataset", str(tmp_path / "base.fvecs"),
            "--eigen", str(tmp_path / "eig.f32"), "--timeseries-size", str(D), "--save", str(tmp_path / "c.bin")]
    r = subprocess.run(args + ["--kmeans-ver", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "iterations " + " ".join(map(str, want[2])) in r.stdout
    got = io.load_centroids(str(tmp_path / "c.bin"))
    for s in range(M):
        cr.assert_centres_equal(got[s], want[1][s], f"demo --kmeans-ver 1, subspace {s}")
    r = subprocess.run(args + ["--kmeans-ver", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "binary k-means is not built" in r.stdout + r.stderr
