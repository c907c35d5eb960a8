"""The CPU side of option "exact_ties" on sequential-sum (BitVecEngine::queryLUT) indexes: the restatements
of libstdc++'s heap functions -- vaq::stdheap in vaq_amd/csrc/vaq_restated.h, which the replay kernel runs, and
seq_exact_ref's Python one -- against the real functions, and against the fixtures under
tests/golden/seq_exact/ (recorded from the loop of BitVecEngine.hpp:1282-1317 over the real functions).  Beside them the reference's own
heap, vaq::refheap in the same header (byte-code and TI indexes), against the oracle's."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import seq_exact_ref as sr


@functools.lru_cache(maxsize=None)
def inputs(name):
    return sr.make_inputs(name)


@functools.lru_cache(maxsize=None)
def all_dists(name):
    """float32 [N_QUERIES][N_ROWS]: a row's distance does not depend on the rows after it"""
    bits, cent, codes, X = inputs(name)
    return np.stack([sr.row_dists(X[q], bits, cent, codes) for q in range(sr.N_QUERIES)])


def shapes():
    return [(k, n) for k in sr.KS for n in sr.row_counts(k)]


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_fixture_inputs_are_the_regenerated_ones(name):
    z = sr.load_fixture(name)
    assert str(z["inputs_digest"]) == sr.digest(*inputs(name))
    assert {f"labels_n{n}_k{k}" for k, n in shapes()} | {f"dists_n{n}_k{k}" for k, n in shapes()} | \
        {"inputs_digest"} == set(z.files)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_restatement_gives_the_recorded_answers(name):
    z = sr.load_fixture(name)
    d = all_dists(name)
    for k, n in shapes():
        want_l, want_d = z[f"labels_n{n}_k{k}"], z[f"dists_n{n}_k{k}"]
        assert want_l.shape == (sr.N_QUERIES, k) and want_l.dtype == np.int32 and want_d.dtype == np.float32
        for q in range(sr.N_QUERIES):
            lab, dis = sr.query_lut_topk(d[q, :n], k)
            assert np.array_equal(lab, want_l[q]), (name, k, n, q)
            assert np.array_equal(dis.view(np.uint32), want_d[q].view(np.uint32)), (name, k, n, q)
            # the answer is a top k of the rows whatever the tie order: the distances are the sorted ones
            assert np.array_equal(dis, sr.smallest_label_topk(d[q, :n], k)[1]), (name, k, n, q)


@pytest.mark.parametrize("name", sr.TIE_HEAVY)
def test_tie_heavy_fixtures_differ_from_the_smallest_label_rule(name):
    """Otherwise the GPU test would pass on the scan's own order.  Every shape with k > 1 (N = k - 1 and
    N = k included: sort_heap's order among equal distances is not the label order), and k = 1 on two rows
    (two equal rows: the pop at row 1 takes the heap's front, row 0)."""
    z = sr.load_fixture(name)
    d = all_dists(name)
    for k, n in shapes():
        differ = sum(int(not np.array_equal(sr.smallest_label_topk(d[q, :n], k)[0], z[f"labels_n{n}_k{k}"][q]))
                     for q in range(sr.N_QUERIES))
        if k > 1 or n == 2:
            assert differ >= 1, (name, k, n)
    assert np.all(z["labels_n2_k1"] == 1)


def heap_sequences():
    """(n, k, float32 keys): random and tie-heavy (2 to 5 distinct keys), the lengths of the issue"""
    rng = np.random.default_rng(20240611)
    out = []
    for n in (1, 2, 3, 16, 17, 101, 1024, 1025):
        for k in sorted({1, 2, 7, 16, 100, max(1, n - 1), n, n + 1}):
            out.append((n, k, rng.normal(size=n).astype(np.float32)))
            for distinct in (2, 3, 4, 5):
                out.append((n, k, rng.integers(0, distinct, n).astype(np.float32)))
        out.append((n, 3, np.zeros(n, np.float32)))
        out.append((n, 3, np.arange(n, dtype=np.float32)))
        out.append((n, 3, np.arange(n, dtype=np.float32)[::-1].copy()))
    return out


def test_stdheap_restatements_match_libstdcxx(tmp_path):
    """vaq::stdheap (built for the host) against std::push_heap / std::pop_heap / std::sort_heap over
    queryLUT's element and comparator, element for element after every call (tests/cpp/stdheap_test.cpp),
    and seq_exact_ref's loop against the ids the real functions return."""
    seqs = heap_sequences()
    assert {n for n, _, _ in seqs} == {1, 2, 3, 16, 17, 101, 1024, 1025}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / "stdheap_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(root, "vaq_amd", "csrc"), os.path.join(root, "tests", "cpp", "stdheap_test.cpp"),
                           "-o", exe])
    with open(str(tmp_path / "in.bin"), "wb") as f:
        np.array([len(seqs)], np.int32).tofile(f)
        for n, k, keys in seqs:
            np.array([n, k], np.int32).tofile(f)
            keys.tofile(f)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"stdheap_test: ok ({len(seqs)} sequences)" in r.stdout
    ids = np.fromfile(str(tmp_path / "out.bin"), np.int32)
    at = 0
    for n, k, keys in seqs:
        m = int(ids[at])
        assert m == min(k, n)
        want = ids[at + 1:at + 1 + m]
        at += 1 + m
        lab, dis = sr.query_lut_topk(keys, k)
        assert np.array_equal(lab[:m], want) and np.all(lab[m:] == -1), (n, k)
        assert np.array_equal(dis[:m], keys[want]) and np.all(np.diff(dis[:m]) >= 0), (n, k)
    assert at == ids.size


def test_refheap_restatement_matches_the_oracle_heap(tmp_path):
    """vaq::refheap (built for the host) against vo_heap_* of oracle/vaq_oracle.c, slot for slot after every call of
    heapify, VAQ::searchHeap's loop and reorder (tests/cpp/refheap_test.cpp): ties and n < k (neutral entries
    dropped by reorder) included.  Run once more under AddressSanitizer + UBSan (host code only, its own main)."""
    seqs = heap_sequences()
    assert {n for n, _, _ in seqs} == {1, 2, 3, 16, 17, 101, 1024, 1025}
    for n in (1, 2, 3, 16, 17, 101, 1024, 1025):
        assert {1, max(1, n - 1), n, n + 1} <= {k for m, k, _ in seqs if m == n}
    assert any(n < k and len(np.unique(keys)) < n for n, k, keys in seqs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx, cc = shutil.which("g++"), shutil.which("gcc")
    assert cxx and cc
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    with open(str(tmp_path / "in.bin"), "wb") as f:
        np.array([len(seqs)], np.int32).tofile(f)
        for n, k, keys in seqs:
            np.array([n, k], np.int32).tofile(f)
            keys.tofile(f)
    for extra, name in ((["-O2"], "refheap_test"),
                        (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "refheap_asan")):
        obj = str(tmp_path / (name + "_oracle.o"))
        subprocess.check_call([cc, "-std=c11", "-g", "-ffp-contract=off"] + extra +
                              ["-c", os.path.join(root, "oracle", "vaq_oracle.c"), "-o", obj])
        exe = str(tmp_path / name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                               "-I" + os.path.join(root, "vaq_amd", "csrc"), "-I" + os.path.join(root, "oracle")] + extra +
                              [os.path.join(root, "tests", "cpp", "refheap_test.cpp"), obj, "-lm", "-o", exe])
        r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert f"refheap_test: ok ({len(seqs)} sequences)" in r.stdout
