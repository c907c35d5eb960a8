"""The CPU side of the exhaustive form across the shards of a multi-device refiner (vaqhip_multi_refiner_search): the
property of the integer rows tests/test_exhaustive_multi_gpu.py relies on, the hand-over of the reference's heap
between the links of the "exact_ties" chain (tests/cpp/refheap_chain_test.cpp), and the refusals that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import refine_ref as rr

MAX_K = 1024
SHARDS = (2, 3, 8)  # G of the GPU test's integer case


def test_integer_inputs_tie_across_the_cuts():
    """int_data() of test_exhaustive_gpu.py under the multi refiner's cut (shards of ceil(N / G) rows): for every G
    used, every query and every k of INT_KS the k-th smallest distance equals the (k + 1)-th, and the rows at that
    distance lie in at least two shards -- a flag or a replay per shard, merged afterwards, cannot give the
    reference's answer there."""
    import test_exhaustive_gpu as g
    Xq, Xt = g.int_data()
    N = len(Xt)
    cand = np.tile(np.arange(N, dtype=np.int32), (len(Xq), 1))
    d = rr.distances(Xq, Xt, cand)
    for G in SHARDS:
        per = -(-N // G)
        shard = np.arange(N) // per
        for q in range(len(Xq)):
            for k in g.INT_KS:
                assert rr.boundary_ties(d[q], k), (G, q, k)
                kth = np.sort(d[q])[k - 1]
                assert len(set(shard[d[q] == kth])) >= 2, (G, q, k)


def test_heap_hand_over(tmp_path):
    """tests/cpp/refheap_chain_test.cpp: vaq::refheap over a sequence in one go equals the same walk with the raw
    arrays handed over at every cut of 2, 3 and 8 parts (empty parts included), for k in {1, 2, 10, 100}, integer
    sequences with many ties, sequences shorter than k and sequences holding inf / NaN; once more under
    AddressSanitizer + UBSan as a stand-alone program."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = os.path.join(root, "tests", "cpp", "refheap_chain_test.cpp")
    text = open(src).read()
    assert "{1, 2, 10, 100}" in text and "{2, 3, 8}" in text
    for extra, exe_name in ((["-O2"], "refheap_chain_test"),
                            (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "refheap_chain_asan")):
        exe = str(tmp_path / exe_name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert "refheap_chain_test: ok (144 sequences x 3 cuts)" in r.stdout


def test_refusals_without_a_device(vaqlib):
    """refused before the refiner or any device is touched: EINVAL (-1) / EUNSUPPORTED (-2)"""
    for name in ("vaqhip_multi_refiner_search", "vaqhip_multi_refiner_search_device",
                 "vaqhip_multi_refiner_last_search_timing"):
        assert hasattr(vaqlib, name), name
    assert vaqlib.vaqhip_version() >= 114
    p = C.c_void_p(64)  # never dereferenced on these paths
    f, fd = vaqlib.vaqhip_multi_refiner_search, vaqlib.vaqhip_multi_refiner_search_device
    assert f(p, p, 4, 0, p, p) == -1
    assert f(p, p, 4, MAX_K + 1, p, p) == -2 and b"1024" in vaqlib.vaqhip_multi_last_error()
    assert f(p, p, 4, 10, None, p) == -1
    assert f(p, p, 4, 10, p, None) == -1
    assert f(p, None, 4, 10, p, p) == -1
    assert f(None, p, 4, 10, p, p) == -1
    assert f(p, p, -1, 10, p, p) == -1
    assert f(p, None, 0, 10, None, None) == 0  # nq == 0 succeeds and touches nothing
    assert fd(p, p, 4, 0, p, p, None) == -1
    assert fd(p, p, 4, MAX_K + 1, p, p, None) == -2
    assert fd(p, p, 4, 10, None, p, None) == -1
    assert fd(p, None, 0, 10, None, None, None) == 0
    from vaq_amd import _lib
    assert vaqlib.vaqhip_multi_refiner_last_search_timing(None, C.byref(_lib.MultiRefinerSearchTiming())) == -1
    assert vaqlib.vaqhip_multi_refiner_last_search_timing(p, None) == -1
    so = vaqlib.vaqhip_multi_refiner_set_option
    assert so(p, b"exhaustive_splits", 65) == -1
    assert b"exhaustive_splits" in vaqlib.vaqhip_multi_last_error()
    assert so(p, b"exhaustive_splits", -1) == -1
    assert so(p, b"no_such_option", 1) == -1
