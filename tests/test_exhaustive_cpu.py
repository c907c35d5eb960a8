"""The CPU side of the exhaustive form of the resident refiner (vaqhip_refiner_search): the per-pair distance its
kernels share with the host (vaq_amd/csrc/vaq_exhaust.h) against vaq::sq_norm_eigen, the properties of the inputs
tests/test_exhaustive_gpu.py relies on, and the refusals that need no device."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import refine_ref as rr

MAX_K = 1024


def test_pair_function_is_sq_norm_eigen(tmp_path):
    """tests/cpp/exhaust_pair_test.cpp: xs_pair_sq_norm == sq_norm_eigen bit for bit for D in {1, 7, 8, 12, 15, 16, 17,
    24, 40, 100, 128, 129, 960}, random floats and rows with NaN / inf; once more under AddressSanitizer + UBSan as a
    stand-alone program."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = os.path.join(root, "tests", "cpp", "exhaust_pair_test.cpp")
    text = open(src).read()
    for D in (1, 7, 8, 12, 15, 16, 17, 24, 40, 100, 128, 129, 960):
        assert f" {D}," in text or f" {D}}}" in text, D
    for extra, exe_name in ((["-O2"], "exhaust_pair_test"),
                            (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "exhaust_pair_asan")):
        exe = str(tmp_path / exe_name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert "exhaust_pair_test: ok (5200 pairs)" in r.stdout


def test_integer_inputs_tie_at_every_k():
    """the integer rows of test_exhaustive_gpu.py over ALL rows: every query has a tie across the k-th slot at every
    tested k, somewhere the heap's labels are not the (distance, label) rule's, and the pinned draw is the first
    that gives this"""
    import test_exhaustive_gpu as g

    def ties(draw):
        Xq, Xt = g.int_data(draw)
        cand = np.tile(np.arange(len(Xt), dtype=np.int32), (len(Xq), 1))
        d = rr.distances(Xq, Xt, cand)
        assert np.array_equal(d, np.round(d))
        return d, cand, all(rr.boundary_ties(d[q], k) for q in range(len(Xq)) for k in g.INT_KS)
    assert not any(ties(draw)[2] for draw in range(g.INT_DRAW))
    d, cand, ok = ties(g.INT_DRAW)
    assert ok
    differ = sum(not np.array_equal(rr.heap_topk(d[q], cand[q], k)[0], rr.smallest_label_topk(d[q], cand[q], k)[0])
                 for q in range(len(d)) for k in g.INT_KS)
    assert differ > 0


def test_mixed_inputs_hold_both_phase_a_outcomes():
    """the mixed batch of test_exhaustive_gpu.py: its first four queries have no two equal distances among their
    first k + 1 (the flag step copies them out), its last four have (they are replayed)"""
    import test_exhaustive_gpu as g
    Xq, Xt = g.mixed_data()
    k = g.MIXED_K
    cand = np.tile(np.arange(len(Xt), dtype=np.int32), (len(Xq), 1))
    d = rr.distances(Xq, Xt, cand)
    # two equal distances among the first k + 1: a tie across slot j for some j <= k
    tied = [any(rr.boundary_ties(d[q], j) for j in range(1, k + 1)) for q in range(len(Xq))]
    assert tied == [False] * 4 + [True] * 4


def test_k_limit_inputs_tie():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(40, 16)).astype(np.float32)
    Xt = base[rng.integers(0, 40, 1500)]
    Xq = rng.integers(0, 256, size=(3, 16)).astype(np.float32)
    cand = np.tile(np.arange(1500, dtype=np.int32), (3, 1))
    d = rr.distances(Xq, Xt, cand)
    for k in (1023, 1024):
        assert all(rr.boundary_ties(d[q], k) for q in range(3)), k


def test_refusals_without_a_device(vaqlib):
    """refused before the refiner or any device is touched: EINVAL (-1) / EUNSUPPORTED (-2)"""
    for name in ("vaqhip_refiner_search", "vaqhip_refiner_search_device", "vaqhip_refiner_last_search_timing"):
        assert hasattr(vaqlib, name), name
    assert vaqlib.vaqhip_version() >= 113
    p = C.c_void_p(64)  # never dereferenced on these paths
    f, fd = vaqlib.vaqhip_refiner_search, vaqlib.vaqhip_refiner_search_device
    assert f(p, p, 4, 0, p, p) == -1
    assert f(p, p, 4, MAX_K + 1, p, p) == -2 and b"1024" in vaqlib.vaqhip_last_error()
    assert f(p, p, 4, 10, None, p) == -1
    assert f(p, p, 4, 10, p, None) == -1
    assert f(p, None, 4, 10, p, p) == -1
    assert f(None, p, 4, 10, p, p) == -1
    assert f(p, p, -1, 10, p, p) == -1
    assert fd(p, p, 4, 0, p, p, None) == -1
    assert fd(p, p, 4, MAX_K + 1, p, p, None) == -2
    assert fd(p, p, 4, 10, None, p, None) == -1
    assert vaqlib.vaqhip_refiner_set_option(p, b"exhaustive_splits", 65) == -1
    assert b"exhaustive_splits" in vaqlib.vaqhip_last_error()
    assert vaqlib.vaqhip_refiner_set_option(p, b"exhaustive_splits", -1) == -1
    assert vaqlib.vaqhip_refiner_set_option(p, b"no_such_option", 1) == -1
