"""The CPU side of the resident refiner: tests/refine_ref.py (a NumPy restatement of VAQ::refine, VAQ.cpp:849-876,
with Eigen's summation order and the reference's heap) and the code the refine kernel shares with the host
(vaq::sq_norm_eigen, vaq::refheap in vaq_amd/csrc/vaq_restated.h) against the fixtures recorded from the reference
itself (tests/golden/refine/README.md)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import refine_ref as rr

CASES = sorted(rr.CASES)
# a continuous fixture on which the summation order of squaredNorm decides labels (see the README)
ORDER_CASE = "cont_d128"


@functools.lru_cache(maxsize=None)
def inputs(name):
    return rr.make_inputs(name)


@functools.lru_cache(maxsize=None)
def dists(name, order="eigen"):
    return rr.distances(*inputs(name), order=order)


def recorded(name, k):
    z = rr.load_fixture(name)
    return z[f"labels_k{k}"], z[f"dists_k{k}"]


def restated(name, k, order="eigen"):
    cand = inputs(name)[2]
    d = dists(name, order)
    out = [rr.heap_topk(d[q], cand[q], k) for q in range(len(cand))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("name", CASES)
def test_inputs_are_the_recorded_ones(name):
    z = rr.load_fixture(name)
    c = rr.CASES[name]
    assert str(z["inputs_digest"]) == rr.digest(*inputs(name)), "numpy no longer generates the recorded inputs"
    assert set(z.files) == {"inputs_digest"} | {f"labels_k{k}" for k in c["ks"]} | {f"dists_k{k}" for k in c["ks"]}
    for k in c["ks"]:
        lab, dis = recorded(name, k)
        assert lab.shape == dis.shape == (c["nq"], k) and lab.dtype == np.int32 and dis.dtype == np.float32


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    for k in rr.CASES[name]["ks"]:
        want_l, want_d = recorded(name, k)
        lab, dis = restated(name, k)
        assert np.array_equal(dis.view(np.uint32), want_d.view(np.uint32)), (name, k)
        assert np.array_equal(lab, want_l), (name, k)


def test_fixtures_cover_the_reduction_and_the_heap():
    """Every path of Eigen's reduction; an integer case on which EVERY query has a tie across the k-th slot for every
    k < R, and on which the heap's labels are not the (distance, label) rule's; duplicates; R = 1 and R = 2048."""
    assert {rr.CASES[n]["D"] for n in rr.CONTINUOUS} == {7, 8, 12, 16, 40, 100, 128, 129, 960}
    c = rr.CASES["int_ties"]
    assert c["N"] == 300 and c["R"] == 200 and set(c["ks"]) == {1, 10, 100, 200} and c["distinct"] == 20
    Xq, Xt, cand = inputs("int_ties")
    assert np.array_equal(Xt, np.round(Xt)) and len(np.unique(Xt, axis=0)) <= 20
    d = dists("int_ties")
    assert np.array_equal(d, dists("int_ties", "sequential"))  # integer data: the order of the sum is harmless
    for k in (1, 10, 100):
        assert all(rr.boundary_ties(d[q], k) for q in range(c["nq"])), k
    for k in c["ks"]:
        sl = np.stack([rr.smallest_label_topk(d[q], cand[q], k)[0] for q in range(c["nq"])])
        assert not np.array_equal(sl, recorded("int_ties", k)[0]), k
    dup = inputs("dup_cands")[2]
    assert all(len(np.unique(row)) < len(row) for row in dup)
    lab64 = recorded("dup_cands", 64)[0]
    assert all(len(np.unique(row)) < len(row) for row in lab64), "the reference keeps duplicate candidates"
    assert rr.CASES["r1"]["R"] == 1 and rr.CASES["r2048"]["R"] == 2048


def test_summation_order_is_pinned_by_data():
    """The sequential sum gives other distances on continuous data from D = 8 on (none below), and on this fixture
    another label list than the reference's: the order of squaredNorm is not a free choice."""
    assert np.array_equal(dists("cont_d7").view(np.uint32), dists("cont_d7", "sequential").view(np.uint32))
    for name in rr.CONTINUOUS:
        if rr.CASES[name]["D"] >= 8:
            assert not np.array_equal(dists(name).view(np.uint32), dists(name, "sequential").view(np.uint32)), name
    for k in rr.CASES[ORDER_CASE]["ks"]:
        want_l, want_d = recorded(ORDER_CASE, k)
        seq_l, seq_d = restated(ORDER_CASE, k, "sequential")
        assert not np.array_equal(seq_l, want_l), k
        assert np.array_equal(restated(ORDER_CASE, k)[0], want_l), k


def test_skipped_labels_in_the_restatement():
    """negative, below id_base, past the end: never admitted, the rest unchanged"""
    Xq, Xt, cand = inputs("cont_d40")
    k = 10
    clean_l, clean_d = rr.refine(Xq, Xt, cand + 1000, k, id_base=1000)
    assert np.array_equal(clean_l - 1000, recorded("cont_d40", k)[0])
    mixed = np.insert(cand + 1000, [0, 5, 50, 200], [-7, 999, 1300, 2**31 - 1], axis=1).astype(np.int32)
    lab, dis = rr.refine(Xq, Xt, mixed, k, id_base=1000)
    assert np.array_equal(lab, clean_l) and np.array_equal(dis, clean_d)
    lab, dis = rr.refine(Xq, Xt, np.full((len(Xq), 3), -1, np.int32), 2)
    assert np.all(lab == -1) and np.all(dis == rr.FLT_MAX)


def test_shared_host_code_matches_the_reference(tmp_path):
    """vaq::sq_norm_eigen and vaq::refheap, the very functions the kernel file uses, built for the host and run as
    VAQ::refine's loop over every fixture (tests/cpp/refine_order_test.cpp); once more under AddressSanitizer +
    UBSan as a stand-alone program."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    n_cases = 0
    with open(str(tmp_path / "in.bin"), "wb") as f:
        np.array([sum(len(rr.CASES[n]["ks"]) for n in CASES)], np.int32).tofile(f)
        for name in CASES:
            c = rr.CASES[name]
            Xq, Xt, cand = inputs(name)
            for k in c["ks"]:
                np.array([c["nq"], c["D"], c["N"], c["R"], k], np.int32).tofile(f)
                Xq.tofile(f)
                Xt.tofile(f)
                cand.tofile(f)
                lab, dis = recorded(name, k)
                lab.tofile(f)
                dis.tofile(f)
                n_cases += 1
    for extra, exe_name in ((["-O2"], "refine_order_test"),
                            (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "refine_order_asan")):
        exe = str(tmp_path / exe_name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [os.path.join(root, "tests", "cpp", "refine_order_test.cpp"), "-o", exe])
        r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert f"refine_order_test: ok ({n_cases} cases)" in r.stdout
