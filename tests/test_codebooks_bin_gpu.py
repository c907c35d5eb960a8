"""The binary-tree codebook fit on the GPU (vaqhip_fit_codebooks_bin*; vaq_amd/csrc/vaq_codebooks.hip): subspaces above
8 bits as a tree of 2-centre fits, splits and cuts, against the composition of the pinned numpy restatements
(tests/codebooks_bin_ref.py).  Every comparison is on bit patterns (NaN by position), plus the iteration counts, the
NaN centres per subspace and the tree's counts -- the GPU took the reference's decisions, not merely the same centres."""
import ctypes as C
import functools

import numpy as np
import pytest

import codebooks_bin_ref as br
import codebooks_hier_ref as hr
import codebooks_ref as cr
from test_codebooks_gpu import PATTERN, _p, host_fit as flat_host_fit, same_fit, split

pytestmark = pytest.mark.gpu

TREE_FIELDS = ("levels", "nodes", "cut_nodes", "leaf_nodes", "resampled_fits", "min_leaf_rows", "max_leaf_rows")


def bin_fit(L_, X, M, bits, eig=None, max_iter=cr.MAX_ITER):
    """vaqhip_fit_codebooks_bin (or its _u8 twin): (rc, [M centre matrices], iterations, nan rows)"""
    return flat_host_fit(L_, X, M, bits, eig, max_iter,
                         fn=L_.vaqhip_fit_codebooks_bin_u8 if X.dtype == np.uint8 else L_.vaqhip_fit_codebooks_bin)


def bin_device_fit(L_, d_X, n, D, M, bits, eig=None, max_iter=cr.MAX_ITER):
    import torch
    ks = [1 << b for b in bits]
    d_cent = torch.full((sum(ks) * (D // M),), float(PATTERN), dtype=torch.float32, device="cuda")
    d_eig = torch.from_numpy(eig).cuda() if eig is not None else None
    iters, nan = np.full(M, -9, np.int32), np.full(M, -9, np.int32)
    fn = L_.vaqhip_fit_codebooks_bin_u8_device if d_X.dtype == torch.uint8 else L_.vaqhip_fit_codebooks_bin_device
    torch.cuda.synchronize()
    rc = fn(0, C.c_void_p(d_X.data_ptr()), n, D, M, (C.c_int * M)(*bits),
            C.c_void_p(d_eig.data_ptr()) if d_eig is not None else None, max_iter, C.c_void_p(d_cent.data_ptr()),
            _p(iters), _p(nan), None)
    return rc, split(d_cent.cpu().numpy(), D, M, bits), iters, nan


def as_fit(expected):
    """the oracle's answer in the shape of bin_fit's"""
    cents, iters, nans, trees = expected
    return 0, cents, np.array(iters, np.int32), np.array([int(m.sum()) for m in nans], np.int32)


@functools.lru_cache(maxsize=None)
def fitted(name):
    """the host form's answer for a case and the figures of that call, computed once (the staged sums: the default)"""
    import vaq_amd
    from vaq_amd import _lib
    n, D, M, bits, kind, salt = br.CASES[name]
    X, eig = br.inputs(name)
    got = bin_fit(_lib.load(), X, M, bits, eig)
    return got, vaq_amd.last_fit_codebooks_bin_timing()


@pytest.mark.parametrize("name", list(br.CASES))
def test_cases_against_the_oracle(vaqlib, name):
    """Every case of the table: centres bit for bit, the largest iteration count among a subspace's fits, the NaN
    centres, and the tree's counts from the timing call."""
    n, D, M, bits, kind, salt = br.CASES[name]
    got, t = fitted(name)
    assert got[0] == 0, vaqlib.vaqhip_last_error()
    same_fit(got, as_fit(br.expected(name)), name)
    want = br.tree_stats(list(br.expected(name)[3].values()))
    assert {f: t[f] for f in TREE_FIELDS} == want
    assert t["bin_subspaces"] == len(br.expected(name)[3]) and t["subspaces"] == M and t["rows"] == n and t["dims"] == D
    assert t["max_iterations"] == max(got[2])


@pytest.mark.parametrize("name", list(br.CASES))
def test_one_thread_sums_give_the_same_bits(vaqlib, name):
    """vaqhip_fit_codebooks_bin_set_sums(1): the flat fit's one-thread-per-run kernel in place of the staged one."""
    n, D, M, bits, kind, salt = br.CASES[name]
    X, eig = br.inputs(name)
    want, _ = fitted(name)
    assert vaqlib.vaqhip_fit_codebooks_bin_set_sums(1) == 0
    try:
        got = bin_fit(vaqlib, X, M, bits, eig)
    finally:
        assert vaqlib.vaqhip_fit_codebooks_bin_set_sums(0) == 0
    same_fit(got, want, name + " with set_sums(1)")
    assert vaqlib.vaqhip_fit_codebooks_bin_set_sums(2) == -1


def test_flat_subspace_beside_a_binary_one(vaqlib):
    """`tiny`: subspace 1 (3 bits) equals vaqhip_fit_codebooks's subspace 1; subspace 0 does not (it is binary)."""
    n, D, M, bits, kind, salt = br.CASES["tiny"]
    X, _ = br.inputs("tiny")
    flat = flat_host_fit(vaqlib, X, M, bits)
    got, _ = fitted("tiny")
    assert flat[0] == 0 and got[0] == 0
    cr.assert_centres_equal(got[1][1], flat[1][1], "flat subspace of tiny")
    assert got[2][1] == flat[2][1] and got[3][1] == flat[3][1]
    assert not np.array_equal(got[1][0], flat[1][0])


@pytest.mark.parametrize("name", ["bytes", "odd"])
def test_no_wide_subspace_is_the_flat_fit(vaqlib, name):
    """All bits <= 8: vaqhip_fit_codebooks's result bit for bit."""
    import vaq_amd
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = cr.make_inputs(name)
    want = flat_host_fit(vaqlib, X, M, bits, eig)
    assert want[0] == 0
    same_fit(bin_fit(vaqlib, X, M, bits, eig), want, name + " through the binary call")
    assert vaq_amd.last_fit_codebooks_bin_timing()["bin_subspaces"] == 0


def test_forms_agree_on_two(vaqlib):
    """`two` through the _device form, the refiner and the Python call."""
    import torch
    import vaq_amd
    n, D, M, bits, kind, salt = br.CASES["two"]
    X, eig = br.inputs("two")
    want, _ = fitted("two")
    assert want[0] == 0, vaqlib.vaqhip_last_error()
    same_fit(bin_device_fit(vaqlib, torch.from_numpy(X).cuda(), n, D, M, bits, eig), want, "two _device")
    r = vaq_amd.VaqRefiner(D)
    r.set_rows(X)
    cents, iters, nan = r.fit_codebooks_bin(M, bits, eig)
    r.close()
    same_fit((0, cents, iters, nan), want, "two refiner")
    cents, iters, nan = vaq_amd.fit_codebooks_bin(X, M, bits, eig)
    same_fit((0, cents, iters, nan), want, "vaq_amd.fit_codebooks_bin")
    t = vaq_amd.last_fit_codebooks_bin_timing()
    assert t["bin_subspaces"] == 2 and t["subspaces"] == M and t["rows"] == n


def test_byte_rows_are_the_widened_rows(vaqlib):
    """`two`'s shape as uint8 rows with values 0..255 behind its eigvec: _u8, _u8_device and the refiner over byte rows
    equal the float call on the widened rows, which equals the oracle."""
    import torch
    import vaq_amd
    n, D, M, bits, kind, salt = br.CASES["two"]
    X8, eig = br.byte_inputs()
    want = bin_fit(vaqlib, X8.astype(np.float32), M, bits, eig)
    assert want[0] == 0, vaqlib.vaqhip_last_error()
    same_fit(want, as_fit(br.expected_bytes()), "widened bytes")
    same_fit(bin_fit(vaqlib, X8, M, bits, eig), want, "two _u8")
    same_fit(bin_device_fit(vaqlib, torch.from_numpy(X8).cuda(), n, D, M, bits, eig), want, "two _u8_device")
    r = vaq_amd.VaqRefiner(D)
    r.set_rows_u8(X8)
    got = r.fit_codebooks_bin(M, bits, eig)
    r.close()
    same_fit((0,) + tuple(got), want, "two refiner, byte rows")
    got = vaq_amd.fit_codebooks_bin_u8(X8, M, bits, eig)
    same_fit((0,) + tuple(got), want, "vaq_amd.fit_codebooks_bin_u8")


def test_refusals_leave_the_outputs(vaqlib):
    """rows_s < k_s for a binary subspace, and a refusal of the flat fit (bits out of range): refused before any device
    work, the outputs keep their contents.  Few distinct slices under a 9-bit subspace -- what the hierarchical form
    refuses -- is fitted."""
    rng = np.random.default_rng(5)
    few = rng.normal(size=(100, 2)).astype(np.float32)
    X = np.ascontiguousarray(np.concatenate([rng.normal(size=(2000, 2)).astype(np.float32), few[rng.integers(0, 100, 2000)]], axis=1))
    rc, cents, iters, nan = bin_fit(vaqlib, X[:300], 2, (3, 9))
    assert rc == -1 and b"out of bounds" in vaqlib.vaqhip_last_error()
    assert all(np.all(c == PATTERN) for c in cents) and np.all(iters == -9) and np.all(nan == -9)
    rc, cents, iters, nan = bin_fit(vaqlib, X, 2, (3, 16))
    assert rc == -1
    assert all(np.all(c == PATTERN) for c in cents) and np.all(iters == -9) and np.all(nan == -9)
    rc, cents, iters, nan = bin_fit(vaqlib, X, 2, (3, 9), max_iter=0)
    assert rc == -1 and all(np.all(c == PATTERN) for c in cents)
    got = bin_fit(vaqlib, X, 2, (3, 9))
    assert got[0] == 0, vaqlib.vaqhip_last_error()
    same_fit(got, as_fit(br.fit_codebooks_bin(X, 2, (3, 9))), "100 distinct slices under 9 bits")
    assert got[3][1] > 0  # (centres without a row of their own stay NaN)


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/fit_codebooks_bin_shim_test.cpp over the hierarchical suite's `two` (an input both forms take):
    mBinaryKmeans gives the C call's centres, both flags the hierarchical ones, after setDevices() it is refused."""
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
    exe = str(tmp_path / "fit_codebooks_bin_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "fit_codebooks_bin_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fit_codebooks_bin_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_kmeans_binary(vaqlib, tmp_path):
    """demo_vaqhip --fit-codebooks --kmeans-binary --save: the saved centres are the binary call's; together with
    --kmeans-ver 1 it is refused."""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    n, D, M, bits, kind, salt = br.CASES["two"]
    X, eig = br.inputs("two")
    io.write_vecs(str(tmp_path / "base.fvecs"), X)
    eig.tofile(str(tmp_path / "eig.f32"))
    want, _ = fitted("two")
    args = [exe, "--fit-codebooks", "--bits", ",".join(map(str, bits)), "--dataset", str(tmp_path / "base.fvecs"),
            "--eigen", str(tmp_path / "eig.f32"), "--timeseries-size", str(D), "--save", str(tmp_path / "c.bin")]
    r = subprocess.run(args + ["--kmeans-binary"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "iterations " + " ".join(map(str, want[2])) in r.stdout
    got = io.load_centroids(str(tmp_path / "c.bin"))
    for s in range(M):
        cr.assert_centres_equal(got[s], want[1][s], f"demo --kmeans-binary, subspace {s}")
    r = subprocess.run(args + ["--kmeans-binary", "--kmeans-ver", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "two different fits" in r.stdout + r.stderr
