"""Option "exact_ties" on TI indexes: labels and distances identical to the reference's VAQ::search with
methods TI and TI|EA, slot for slot, against the answers recorded under tests/golden/ti_exact/ (README there).
Labels by np.array_equal, distances bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.helpers import assert_topk_matches

import ti_exact_ref as tr

pytestmark = pytest.mark.gpu


def _index(inp, method, visit, n=None, clusters_first=True, exact=True):
    from vaq_amd.index import NNMethod, VaqHip
    codes = inp["codes"] if n is None else inp["codes"][:n]
    methods = NNMethod.TI | (NNMethod.EA if method == "TI_EA" else 0)
    v = VaqHip()
    v.mBitsAlloc = inp["bits"]
    v.mCentroidsPerSubs = inp["cents"]
    v.mVisit = visit
    v.mTISegmentNum = inp["seg"]
    v.mTIClusterNum = inp["clusters"].shape[0]
    if clusters_first:
        v.mMethods = methods
        v.mTIClusters = inp["clusters"]
        v.mCodebook = codes
    else:  # the reference's order: encode, then clusterTI regroups what is already there
        v.mMethods = NNMethod.Heap
        v.mCodebook = codes
        v.search(inp["X"][:1], 1, projected=True)
        v.mMethods = methods
        v.mTIClusters = inp["clusters"]
    if exact:
        v.set_option("exact_ties", 1)
    return v


def _same(ans, fx, key, nq, k, what, rows=slice(None)):
    lab, dis = ans.labels.reshape(nq, k), ans.distances.reshape(nq, k)
    want_l, want_d = fx["lab_" + key][rows], fx["dis_" + key][rows]
    assert np.array_equal(lab, want_l), what
    assert np.array_equal(dis.view(np.uint32), want_d.view(np.uint32)), what


@pytest.mark.parametrize("clusters_first", [True, False], ids=["clusters_first", "codes_first"])
@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_exact_ties_ti_equals_the_reference(name, clusters_first):
    inp = tr.make_inputs(name)
    fx = tr.load_fixture(name)
    for n in tr.rows_of(name):
        v = _index(inp, "TI_EA", 1.0, n=n, clusters_first=clusters_first)
        for nn, k, visit, method in tr.combos(name):
            if nn != n:
                continue
            from vaq_amd.index import NNMethod
            v.mVisit = visit
            v.mMethods = NNMethod.TI | (NNMethod.EA if method == "TI_EA" else 0)
            ans = v.search(inp["X"], k, projected=True)
            _same(ans, fx, tr.key(n, k, visit, method), tr.N_QUERIES, k, (name, n, k, visit, method))
        v.close()


@pytest.mark.parametrize("name", ["grid", "nan_centres"])
def test_answer_does_not_depend_on_the_batch(name):
    inp = tr.make_inputs(name)
    fx = tr.load_fixture(name)
    n = tr.CASES[name]["N"]
    v = _index(inp, "TI_EA", 0.25)
    for lo, hi in ((0, 5), (5, tr.N_QUERIES)):
        ans = v.search(inp["X"][lo:hi], 100, projected=True)
        _same(ans, fx, tr.key(n, 100, 0.25, "TI_EA"), hi - lo, 100, (name, lo, hi), rows=slice(lo, hi))
    v.close()


def test_k_1024():
    """the option used to stop at k = 1023"""
    inp = tr.make_inputs("cont")
    fx = tr.load_fixture("cont")
    v = _index(inp, "TI_EA", 1.0)
    ans = v.search(inp["X"], tr.K_LARGE, projected=True)
    _same(ans, fx, tr.key(tr.CASES["cont"]["N"], tr.K_LARGE, 1.0, "TI_EA"), tr.N_QUERIES, tr.K_LARGE, "k=1024")
    v.close()


@pytest.mark.parametrize("name", ["grid", "grid_bits"])
def test_rows_appended_invalidate_the_member_order(name):
    inp = tr.make_inputs(name)
    fx = tr.load_fixture(name)
    n = tr.CASES[name]["N"]
    v = _index(inp, "TI_EA", 1.0, n=n // 2)
    v.search(inp["X"], 7, projected=True)  # builds the member order of the first half
    v.add_codes(inp["codes"][n // 2:])
    for method in tr.METHODS:
        from vaq_amd.index import NNMethod
        v.mMethods = NNMethod.TI | (NNMethod.EA if method == "TI_EA" else 0)
        ans = v.search(inp["X"], 100, projected=True)
        _same(ans, fx, tr.key(n, 100, 1.0, method), tr.N_QUERIES, 100, (name, "appended", method))
    v.close()


@pytest.mark.parametrize("method", tr.METHODS)
def test_cpp_shim_cluster_ti_then_search(tmp_path, method):
    """include/vaqhip.hpp: VaqHip with exactTies, codes first, then clusterTI(), then search()"""
    from vaq_amd import build
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ti_exact_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "ti_exact_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    name, k, visit = "grid_bits", 7, 0.25
    inp = tr.make_inputs(name)
    n, M, L = tr.CASES[name]["N"], len(inp["bits"]), tr.CASES[name]["L"]
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.array([M, L, n, inp["clusters"].shape[0], inp["seg"], tr.N_QUERIES, k, method == "TI_EA"],
                         np.int32).tobytes())
        f.write(np.float32(visit).tobytes())
        f.write(np.asarray(inp["bits"], np.int32).tobytes())
        for c in inp["cents"]:
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
        for a in (inp["codes"], inp["clusters"], inp["X"]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ti_exact_shim ok" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(str(tmp_path / "out.bin"), np.int32)
    lab = raw[:tr.N_QUERIES * k].reshape(tr.N_QUERIES, k)
    dis = raw[tr.N_QUERIES * k:].reshape(tr.N_QUERIES, k)
    fx = tr.load_fixture(name)
    assert np.array_equal(lab, fx["lab_" + tr.key(n, k, visit, method)])
    assert np.array_equal(dis.view(np.uint32), fx["dis_" + tr.key(n, k, visit, method)].view(np.uint32))


@pytest.mark.parametrize("name", ["grid", "cont"])
def test_option_off_keeps_the_default_tie_contract(name):
    """the same index with the option switched off again answers as before: the stable-tie restatement under
    the tie contract of the default path"""
    inp = tr.make_inputs(name)
    ti = po.cluster_ti(inp["codes"], inp["cents"], inp["clusters"], inp["seg"])
    v = _index(inp, "TI_EA", 1.0)
    k = 100
    v.search(inp["X"], k, projected=True)
    v.set_option("exact_ties", 0)
    ans = v.search(inp["X"], k, projected=True)
    ol, od, _ = po.search_ti(inp["X"], inp["cents"], ti, k, visit=1.0, projected=True)
    mb = max(inp["bits"])
    alld = np.stack([np.sqrt(po.all_dists(po.create_lut(inp["X"][q], inp["cents"], mb), inp["codes"]))
                     for q in range(tr.N_QUERIES)])
    assert_topk_matches(ans.labels.reshape(tr.N_QUERIES, k), ans.distances.reshape(tr.N_QUERIES, k), ol, od,
                        all_dists=alld, what="option off " + name)
    v.close()
