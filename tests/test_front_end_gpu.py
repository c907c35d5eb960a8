"""What runs in front of the scan: the lookup tables, the cost keys made where table 0 is computed, and the ranking of
the queries (a counting sort whose workgroups each place their own 1024 queries).

Bar: tables bit-equal to the oracle's; keys bit-equal to query_cost_kernel's over the same tables; the order a
permutation of the queries with ascending key classes; labels and distances identical with the ranking on and off.
No tolerance anywhere: every value is integer work or one fixed chain of IEEE operations."""
import os
import subprocess

import numpy as np
import pytest

from helpers import assert_topk_matches, make_case

pytestmark = pytest.mark.gpu

LUT_QT = 8                       # queries per workgroup of the batched table kernel (vaq_front.hip)
COST_ORDER_MIN_QUERIES = 1024    # vaqhip_index.h
QORDER_MAX = 16384               # vaq_front.hip: most queries of one ranking
N_ROWS = 20000
NONUNIFORM = [12, 10, 9, 8, 8, 7, 6, 4]   # a first table of 4096 entries: the key samples its buckets
SHAPES = {"m8": [8] * 8, "nonuniform": NONUNIFORM}
SEEDS = {"m8": 9101, "nonuniform": 9102}
NQ_MAX = 2500
_cases = {}


def make_index(c):
    import vaq_amd
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(c["bits"])
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    return v


def oracle_all_dists(oracle, c, Xp):
    return np.stack([oracle.all_dists(oracle.create_lut(Xp[q], c["cents"], max(c["bits"])), c["codes"])
                     for q in range(Xp.shape[0])])


def _case(name):
    """One set of inputs per shape for the whole module (never modified)."""
    if name not in _cases:
        c = make_case(SEEDS[name], 128, SHAPES[name], N_ROWS, NQ_MAX, dup_frac=0.02)
        c["X"][7] = np.nan            # no valid table: ranks last and still gets its row
        c["X"][11] = c["X"][12]       # identical queries: identical keys
        _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("nq", [2 * LUT_QT, 2 * LUT_QT + 1, 1], ids=["batched", "ragged", "one"])
def test_tables_match_oracle(vaqlib, oracle, name, nq):
    """vaqhip_build_lut == oracle.create_lut after oracle.project: the smallest batched launch, a ragged last tile, and
    the per-query kernel."""
    c = _case(name)
    v = make_index(c)
    X = c["X"][20:20 + nq]
    Xp = oracle.project(X, c["eig"])
    o_lut = np.stack([oracle.create_lut(Xp[q], c["cents"], max(c["bits"])) for q in range(nq)])
    lut = v.build_lut(X)
    assert np.array_equal(lut.view(np.uint32), o_lut.view(np.uint32))
    v.close()


def test_keys_from_table_build_match_standalone(vaqlib, tmp_path):
    """tests/cpp/front_end_keys_test.cpp: for every bucket shift that launch_cost_order takes and for query counts up to
    QORDER_MAX, the table build with keys asked for leaves the same tables and the same 64-bit keys as the table build
    followed by query_cost_kernel, and both rankings are permutations with ascending classes."""
    from vaq_amd import build
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "front_end_keys_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(root, "vaq_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "front_end_keys_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(9200)
    L = 4
    total = 0
    for bits, nqs in (([8] * 8, [2 * LUT_QT, 2 * LUT_QT + 1, COST_ORDER_MIN_QUERIES + 1, QORDER_MAX]),
                      (NONUNIFORM, [2 * LUT_QT + 3, COST_ORDER_MIN_QUERIES + 1]),
                      ([10, 2, 8], [2 * LUT_QT, 257])):     # 1024 entries read back unsampled; a codebook below 8
        n0 = 1 << bits[0]
        shifts = [s for s in range(bits[0] + 1) if 1 <= (n0 >> s) <= 1024]
        M = len(bits)
        X = (rng.normal(size=(max(nqs), M * L)) * 30.0).astype(np.float32)
        X[3] = np.nan
        X[5] = X[6]
        X[9, :L] = np.inf
        with open(str(tmp_path / "in.bin"), "wb") as f:
            f.write(np.array([M, L, len(nqs), len(shifts)], np.int32).tobytes())
            f.write(np.array(bits, np.int32).tobytes())
            f.write(np.array(nqs, np.int32).tobytes())
            f.write(np.array(shifts, np.int32).tobytes())
            for b in bits:   # dimension-major codebooks
                f.write(np.ascontiguousarray((rng.normal(size=(L, 1 << b)) * 30.0).astype(np.float32)).tobytes())
            f.write(X.tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
        want = "front_end_keys ok %d" % (len(nqs) * len(shifts))
        assert r.returncode == 0 and want in r.stdout, r.stdout + r.stderr
        total += len(nqs) * len(shifts)
    assert total > 0


def _search_prefilled(v, X, k, projected=False):
    """search_device into buffers that hold a sentinel: a query nobody answers shows."""
    import torch
    q = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    lab = torch.full((X.shape[0], k), -77, dtype=torch.int32, device="cuda")
    dis = torch.full((X.shape[0], k), -1.0, dtype=torch.float32, device="cuda")
    v.search_device(q, k, projected=projected, out=(lab, dis))
    torch.cuda.synchronize()
    return lab.cpu().numpy(), dis.cpu().numpy()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_ranked_search_equals_unranked(vaqlib, oracle, name):
    """Labels and distances with cost_order 1 and 0 at the smallest ranked call, one more, and 2500 queries."""
    c = _case(name)
    k = 20
    v = make_index(c)
    checked = 32
    Xp = oracle.project(c["X"][:checked], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(c["bits"]), projected=True)
    ad = oracle_all_dists(oracle, c, Xp)
    good = [i for i in range(checked) if i != 7]
    for nq in (COST_ORDER_MIN_QUERIES, COST_ORDER_MIN_QUERIES + 1, NQ_MAX):
        X = c["X"][:nq]
        v.set_option("timing", 1)
        v.set_option("cost_order", 1)
        on_lab, on_dis = _search_prefilled(v, X, k)
        tm = v.last_timing()
        assert tm["best_first"] == 1 and tm["slices"] == 1, tm   # the plan that ranks its queries
        v.set_option("timing", 0)
        v.set_option("cost_order", 0)
        off_lab, off_dis = _search_prefilled(v, X, k)
        assert not (on_lab == -77).any() and not (off_lab == -77).any()
        assert np.array_equal(on_lab, off_lab), nq
        assert np.array_equal(on_dis.view(np.uint32), off_dis.view(np.uint32)), nq
        assert_topk_matches(on_lab[good], on_dis[good], o_lab[good], o_dis[good], ad[good], what=f"{name} ranked nq={nq}")
    v.close()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_projection_variants(vaqlib, oracle, name):
    """With the rotation, without it, and with queries that arrive projected: each against the oracle, in a call
    large enough to be ranked."""
    c = _case(name)
    k, nq, checked = 20, COST_ORDER_MIN_QUERIES + 5, 24
    X = c["X"][:nq]
    good = [i for i in range(checked) if i != 7]
    Xp_all = oracle.project(X, c["eig"])
    for variant in ("rotated", "unrotated", "projected"):
        cc = dict(c, eig=None) if variant == "unrotated" else c
        v = make_index(cc)
        Xq = X if variant != "projected" else Xp_all
        Xp = X[:checked] if variant == "unrotated" else Xp_all[:checked]
        lab, dis = _search_prefilled(v, Xq, k, projected=(variant == "projected"))
        assert not (lab == -77).any(), variant
        o_lab, o_dis = oracle.search(np.ascontiguousarray(Xp), c["cents"], c["codes"], k, max_bits=max(c["bits"]),
                                     projected=True)
        ad = oracle_all_dists(oracle, c, Xp)
        assert_topk_matches(lab[good], dis[good], o_lab[good], o_dis[good], ad[good], what=f"{name} {variant}")
        v.close()
