"""Option "exact_ties" on TI indexes, the parts that need no GPU: the fixtures under tests/golden/ti_exact/
belong to the inputs tests/ti_exact_ref.py regenerates, the tie-heavy cases really separate the reference's
visiting order from the stable one (what makes tests/test_ti_exact_gpu.py fail without the feature), and the
generalised std::sort restatement (vaq::stdsort::sort_by, vaq_restated.h) equals libstdc++'s std::sort under the
two comparators the feature sorts by."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po

import ti_exact_ref as tr


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_fixture_belongs_to_the_regenerated_inputs(name):
    fx = tr.load_fixture(name)
    assert str(fx["inputs_digest"]) == tr.digest(tr.make_inputs(name))
    for n, k, visit, method in tr.combos(name):
        lab, dis = fx["lab_" + tr.key(n, k, visit, method)], fx["dis_" + tr.key(n, k, visit, method)]
        assert lab.shape == dis.shape == (tr.N_QUERIES, k) and lab.dtype == np.int32 and dis.dtype == np.float32
        filled = min(n, k)
        assert np.all(lab[:, :filled] >= 0) and np.all(lab[:, filled:] == -1)
        assert np.all(dis[:, filled:] == np.finfo(np.float32).max)


@pytest.mark.parametrize("name", tr.TIE_HEAVY)
def test_tie_heavy_cases_separate_the_reference_order_from_the_stable_one(name):
    """More than half of the (query, k > 1, method) entries differ from the stable-tie restatement
    (oracle.vo_search_ti_all); without EA some differ as SETS: the member order decides which rows come back."""
    inp = tr.make_inputs(name)
    fx = tr.load_fixture(name)
    ti = po.cluster_ti(inp["codes"], inp["cents"], inp["clusters"], inp["seg"])
    differ = total = set_differs_no_ea = 0
    for n, k, visit, method in tr.combos(name):
        if k == 1:
            continue
        ol, _, _ = po.search_ti(inp["X"], inp["cents"], ti, k, visit=visit, ea=method == "TI_EA", projected=True)
        lab = fx["lab_" + tr.key(n, k, visit, method)]
        total += lab.shape[0]
        differ += int((ol != lab).any(1).sum())
        if method == "TI":
            set_differs_no_ea += sum(set(a.tolist()) != set(b.tolist()) for a, b in zip(ol, lab))
    assert 2 * differ > total, (differ, total)
    assert set_differs_no_ea > 0
    # the shape of the case: a cluster with more than 16 members of equal xcc (introsort partitions), an empty one
    sizes = np.diff(ti["start"])
    assert (sizes == 0).any()
    runs = [np.unique(ti["code2cc"][ti["member"][ti["start"][t]:ti["start"][t + 1]]], return_counts=True)[1].max()
            for t in range(len(sizes)) if sizes[t]]
    assert max(runs) > 16


def test_nan_centres_inputs_shape():
    """(the inputs only: the NaN clusters' places in the order are pinned by the GPU test against the fixture)"""
    inp = tr.make_inputs("nan_centres")
    nan_rows = np.nonzero(np.isnan(inp["clusters"]).any(1))[0]
    T = inp["clusters"].shape[0]
    assert len(nan_rows) == 2 and nan_rows.min() > 0 and nan_rows.max() < T - 1


def _build(tmp_path, extra, exe_name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / exe_name)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                          [os.path.join(root, "tests", "cpp", "stdsort_generic_test.cpp"), "-o", exe])
    return exe


def test_generic_stdsort_matches_libstdcxx(tmp_path):
    """Lengths 0..40, 1000 and 4096; all-equal, few-distinct and NaN-bearing keys; both comparators; the program
    compares element for element and is run once more under AddressSanitizer + UBSan (host code only)."""
    seqs = tr.sort_sequences()
    assert {len(k) for _, k in seqs} >= set(range(0, 41)) | {1000, 4096}
    assert any(m == 1 and np.isnan(k).any() for m, k in seqs) and any(m == 0 and len(np.unique(k)) == 1 for m, k in seqs)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.int32(len(seqs)).tobytes())
        for mode, keys in seqs:
            f.write(np.array([mode, len(keys)], np.int32).tobytes())
            f.write(keys.astype(np.float32).tobytes())
    outs = []
    for extra, exe_name in ((["-O2"], "stdsort_generic_test"),
                            (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "stdsort_generic_asan")):
        exe = _build(tmp_path, extra, exe_name)
        out = str(tmp_path / (exe_name + ".out"))
        r = subprocess.run([exe, str(tmp_path / "in.bin"), out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert f"stdsort_generic_test: ok ({len(seqs)} sequences)" in r.stdout
        outs.append(np.fromfile(out, np.int32))
    assert np.array_equal(outs[0], outs[1])
    at = 0
    for mode, keys in seqs:
        perm = outs[0][at:at + len(keys)]
        at += len(keys)
        assert np.array_equal(np.sort(perm), np.arange(len(keys)))
        if not np.isnan(keys).any():
            assert np.all(np.diff(keys[perm]) <= 0) if mode == 0 else np.all(np.diff(keys[perm]) >= 0)
    assert at == outs[0].size
