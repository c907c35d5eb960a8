"""The checker of the cluster form (tests/bitvec_clusters_ref.py) on an input worked out by hand and on the fixtures the
compiled reference answered (tests/golden/hamming/clusters_*.npz); the refusals the adapter makes before the library is
touched; the inputs of the edge tests (tests/bitvec_clusters_cases.py), whose builders assert their own conditions; and
the plan's fallback sort on the host against the checker's.  Needs no GPU."""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import bitvec_cases as bc
import bitvec_clusters_cases as cc
import bitvec_clusters_ref as cr
import bitvec_ref as br
import vaq_amd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "hamming")


def test_checker_on_a_worked_example():
    """Six rows of one word, query 0, so a row's distance is its popcount:

        row      0  1  2  3  4  5
        bits     3  1  7  1  0  3      distance 2  1  3  1  0  2
        cluster  1  0  1  0  1  0      cluster 0 = rows {1, 3, 5}, cluster 1 = rows {0, 2, 4}

    The original query (0) is nearer to centre 0 (at 1, distance 1) than to centre 1 (at 3, distance 9).

    k = 2, atleast 1: cluster 0 alone holds k rows.  Candidates 1, 3, 5 with distances 1, 1, 2; the head (1, 3) is
    sorted, 5 is not smaller than the last: rows 1, 3.
    k = 2, atleast 2: candidates 1, 3, 5, 0, 2, 4 with distances 1, 1, 2, 2, 3, 0.  Row 4 (distance 0) replaces the
    last of the head and moves to the front: rows 4, 1 -- row 3, equal to row 1, is the one pushed out.
    k = 3, atleast 1: the head is (1, 3, 5) = distances 1, 1, 2; nothing follows: rows 1, 3, 5.
    k = 3, atleast 2: head as before; row 0 (distance 2) ties with the last, row 5, across the cut and stays out;
    row 4 (distance 0) pushes row 5 out: rows 4, 1, 3."""
    rows = np.array([[3], [1], [7], [1], [0], [3]], np.uint64)
    queries = np.zeros((1, 1), np.uint64)
    cen = np.array([[1.0], [3.0]], np.float32)
    idx = np.array([1, 0, 1, 0, 1, 0], np.int32)
    oq = np.zeros((1, 1), np.float32)
    for k, atleast, labels, dists in [(2, 1, [1, 3], [1, 1]), (2, 2, [4, 1], [0, 1]), (3, 1, [1, 3, 5], [1, 1, 2]),
                                      (3, 2, [4, 1, 3], [0, 1, 1])]:
        lab, dis = cr.query_clusters(rows, queries, cen, idx, oq, k, atleast, id_base=10)
        assert lab.tolist() == [[10 + r for r in labels]] and dis.tolist() == [dists], (k, atleast)
    # fewer candidates than k: the slots behind them are empty
    lab, dis = cr.query_clusters(rows, queries, cen, idx, oq, 8, 1)
    assert lab.tolist() == [[4, 1, 3, 5, 0, 2, -1, -1]] and dis[0, 6:].tolist() == [0xffffffff] * 2
    # the rerank form: kTemp = 4 candidates (4, 1, 3, then 5 ahead of its equal 0), reranked by |x - 0|^2
    X = np.array([[9], [2], [9], [1], [3], [1]], np.uint8)
    lab, dis = cr.query_rerank_clusters(rows, queries, cen, idx, X, oq, 2, 2, 2)
    assert lab.tolist() == [[3, 5]] and dis.tolist() == [[1.0, 1.0]]


def test_adapter_refuses_before_the_library():
    bv = vaq_amd.VaqBitVec.__new__(vaq_amd.VaqBitVec)  # (no handle: the refusals come before it is read)
    bv._h, bv.device, bv.n_bits, bv.W = C.c_void_p(), 0, 64, 1
    Q = np.zeros((2, 1), np.uint64)
    calls = [
        lambda: bv.set_clusters(np.zeros(4, np.float32), np.zeros(3, np.int32)),            # centres not T x D
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.zeros(3, np.float32)),     # indices not integers
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.zeros((3, 1), np.int32)),  # not one-dimensional
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.array([0, 2, 1])),         # past the centres
        lambda: bv.set_clusters(np.zeros((2, 4), np.float32), np.array([0, -1, 1])),
    ]
    for call in calls:
        with pytest.raises(vaq_amd.VaqHipError) as e:
            call()
        assert e.value.code == -1
    with pytest.raises(vaq_amd.VaqHipError) as e:  # no cluster state yet
        bv.query_clusters(Q, np.zeros((2, 4), np.float32), 3)
    assert e.value.code == -7
    bv.cluster_D = 4
    for oq in (np.zeros((2, 5), np.float32), np.zeros((3, 4), np.float32)):  # another dimension, another count
        with pytest.raises(vaq_amd.VaqHipError) as e:
            bv.query_clusters(Q, oq, 3)
        assert e.value.code == -1
        with pytest.raises(vaq_amd.VaqHipError) as e:
            bv.query_rerank_clusters(Q, oq, 3, 2, None)
        assert e.value.code == -1


# ---- the inputs of tests/test_bitvec_clusters_edges_gpu.py: every builder of tests/bitvec_clusters_cases.py asserts what
# makes its input worth running; the properties the GPU tests lean on are checked again here

def test_edge_inputs_every_width():
    for W in range(1, 17):
        n_bits, rows, queries, cen, idx, oq = cc.every_width(W)
        assert (n_bits + 63) // 64 == W == rows.shape[1] and (n_bits % 64 != 0) == (W % 2 == 1)
        assert rows.shape[0] == sum(cc.SIZES_A) and queries.shape[0] == oq.shape[0] == 9 and cc.ID_BASE_A != 0
        sizes = np.bincount(idx, minlength=len(cc.SIZES_A))
        assert {0, 1, 255, 256, 257} <= set(sizes.tolist()) and sizes.max() > 512
        cand, d, clu = cc.view(rows, queries, cen, idx, oq, 0, cc.K_A, cc.ATLEAST_A)
        assert cc.crosses(d, cc.K_A) and len(set(clu.tolist())) >= 2


def test_edge_inputs_far_bins():
    # PER of the select kernel at the far widths, and where it first becomes 2: thread 128 owns bin 256 at W = 4
    assert [cc.select_per(W) for W in bc.FAR_WIDTHS] == [1, 1, 2, 3, 4, 5]
    assert [W for W in range(2, 17) if cc.select_per(W) > cc.select_per(W - 1)] == [4, 8, 12, 16]
    assert 64 * 4 // cc.select_per(4) == 128
    for W in bc.FAR_WIDTHS:
        case = cc.far_clusters(W)
        assert sorted(np.bincount(case[3]).tolist()) == sorted(cc.SIZES_B) and max(cc.SIZES_B) > 256
        seen = set()
        for atleast in (len(cc.SIZES_B), 1):
            for off in (0, 1):
                k = cc.far_k(case, off, atleast)
                cc.check_far(case, k, off, atleast)
                cand, d, clu = cc.view(*case, 0, k, atleast)
                assert np.sort(d)[k - 1] == 64 * W - off == np.sort(d)[k]
                assert (len(cand) == 600) == (atleast != 1)
                seen.add(k)
        assert len(seen) == 4
    rows, queries, cen, idx, oq, k = cc.full_head()
    assert k == 1024 and rows.shape == (1100, 8)


def test_edge_inputs_plan():
    assert (cc.CLUSTERS_MAX, 4, 3) in cc.PLAN_SHAPES and (9, cc.CLUSTERS_MAX_DIM, 3) in cc.PLAN_SHAPES
    assert {255, 256, 257, 4095, 4096} <= {s[0] for s in cc.PLAN_SHAPES} & {s[0] for s in cc.PLAN_TIE_SHAPES}
    assert any(4 * D < 8 * T for T, D, _ in cc.PLAN_SHAPES)
    assert any(0 < 8 * T - 4 * D <= 8 for T, D, _ in cc.PLAN_SHAPES) and any(0 < 4 * D - 8 * T <= 8 for T, D, _ in cc.PLAN_SHAPES)
    for T, D, nq in cc.PLAN_SHAPES:
        rows, queries, cen, idx, oq, atleast = cc.plan_shape(T, D, nq, False)
        assert cen.shape == (T, D) and oq.shape == (nq, D) and idx.max() < T
    for T, D, nq in cc.PLAN_TIE_SHAPES:
        rows, queries, cen, idx, oq, atleast = cc.plan_shape(T, D, nq, True)
        d = cc.dists_of(cen, oq)
        assert len(np.unique(d[0])) < T // 2 + 2


def test_edge_inputs_no_fusing():
    """every pair is told apart by the arithmetic: the restatement's labels of query 0 differ under a fused sum"""
    pairs = set()
    for seed in range(4):
        rows, queries, cen, idx, oq = cc.fuse_sensitive(seed)
        a = cr.query_clusters(rows, queries, cen, idx, oq, cc.K_C, 1)
        b = cr.query_clusters(rows, queries, cen, idx, oq, cc.K_C, 1, dist=cc.euclidean_fused)
        assert not np.array_equal(a[0][0], b[0][0])
        pairs.add(cen[:2].tobytes())
    assert len(pairs) == 4
    # the fused form is one rounding where the plain one is two: within an ulp or so of it, and not always equal
    rs = np.random.RandomState(1)
    X, q = rs.standard_normal((1000, 3)).astype(np.float32), rs.standard_normal(3).astype(np.float32)
    f, sure = cc.fused_sums(q, X)
    p = br.euclidean_no_sqrt(q, X)
    assert sure.sum() > 900 and (np.abs(f.astype(np.float64) - p) <= 2 * np.spacing(p)).all() and 50 < (f != p).sum() < 950
    t = (q[0] - X[:, 0]).astype(np.float32)  # D = 1: both are the rounded square of the rounded difference
    assert np.array_equal(cc.fused_sums(q[:1], X[:, :1])[0], (t.astype(np.float64) ** 2).astype(np.float32))
    assert np.array_equal(br.euclidean_no_sqrt(q[:1], X[:, :1]), (t.astype(np.float64) ** 2).astype(np.float32))


def test_edge_inputs_nonfinite_seams_and_state():
    for kind in cc.NONFINITE:
        rows, queries, cen, idx, oq, k, atleast = cc.nonfinite(kind)
        lab, dis = cr.query_clusters(rows, queries, cen, idx, oq, k, atleast)
        assert (lab >= 0).all()
    assert float(np.float32(3e19)) ** 2 > float(br.FLT_MAX)
    rows, queries, X, XQ, cen, idx = cc.small_chunks()
    assert queries.shape[0] == 5 and cc.PER_QUERY_BYTES(len(cen)) == 40
    rows, base, X, XQ7, cen, idx, want, want_rr = cc.seam()
    assert rows.shape == (64, 1) and cen.shape == (4, 4) and want[0].shape == (7, 3) and want_rr[0].shape == (7, 2)
    steps, queries, oq = cc.state_steps()
    assert [s[1].shape for s in steps] == [(300, 4), (3, 4), (300, 4), (40, 9), (7, 9), (300, 4)]


def _build_sort(tmp_path, extra, exe_name):
    root = os.path.dirname(HERE)
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / exe_name)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                          [os.path.join(root, "tests", "cpp", "cluster_sort_test.cpp"), "-o", exe])
    return exe


def test_fallback_sort_is_the_restated_sort(tmp_path):
    """The plan's fallback, stdsort::sort_by<12, true> under ClusterLt, built for the host and run on the centre
    distances of the tie, infinity and NaN cases: the permutation is bitvec_ref.std_sort_perm_f32's, the checker's.
    The program itself holds it against the real std::sort where no NaN is among the distances and against its own
    unguarded form where one is; it runs once more under AddressSanitizer + UBSan (host code only)."""
    arrays = cc.sort_arrays()
    assert any(np.isnan(d).all() for _, d in arrays) and any(np.isnan(d).sum() == 1 for _, d in arrays)
    assert any(np.isinf(d).sum() > 2 for _, d in arrays) and {len(d) for _, d in arrays} >= {9, 40, 255, 256, 257, 4095, 4096}
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.int32(len(arrays)).tobytes())
        for _, d in arrays:
            f.write(np.int32(len(d)).tobytes())
            f.write(d.astype(np.float32).tobytes())
    n_nan = sum(bool(np.isnan(d).any()) for _, d in arrays)
    for extra, exe_name in ((["-O2"], "cluster_sort_test"),
                            (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "cluster_sort_asan")):
        exe = _build_sort(tmp_path, extra, exe_name)
        out = str(tmp_path / (exe_name + ".out"))
        r = subprocess.run([exe, str(tmp_path / "in.bin"), out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert f"cluster_sort_test: ok ({len(arrays)} sequences, {n_nan} with a NaN)" in r.stdout
        got = np.fromfile(out, np.int32)
        at = 0
        for name, d in arrays:
            assert np.array_equal(got[at:at + len(d)], br.std_sort_perm_f32(d)), name
            at += len(d)
        assert at == got.size


# ---- the fixtures of tests/golden/hamming/clusters_*.npz, which the compiled reference's KNNFromDists answered

def cluster_fixtures():
    files = sorted(glob.glob(os.path.join(GOLD, "clusters_*.npz")))
    assert len(files) >= 2
    return [pytest.param(f, id=os.path.basename(f)[:-4]) for f in files]


@pytest.mark.parametrize("path", cluster_fixtures())
def test_checker_matches_fixture(path):
    g = np.load(path)
    k, atleast = int(g["k"]), int(g["atleast"])
    for q in range(g["queries"].shape[0]):
        cand = cr.candidates(g["centroids"], g["clust_idx"], g["XQ"][q], int(g["k_walk"]), atleast)
        assert np.array_equal(cand, g["candidates"][q][:int(g["n_cand"][q])])
    if "factor" in g:
        lab, dis = cr.query_rerank_clusters(g["rows"], g["queries"], g["centroids"], g["clust_idx"], g["X"], g["XQ"], k,
                                            int(g["factor"]), atleast)
        ham, _ = cr.query_clusters(g["rows"], g["queries"], g["centroids"], g["clust_idx"], g["XQ"], int(g["k_walk"]), atleast)
        assert np.array_equal(ham, g["hamming_labels"])
    else:
        lab, dis = cr.query_clusters(g["rows"], g["queries"], g["centroids"], g["clust_idx"], g["XQ"], k, atleast)
    assert np.array_equal(lab, g["labels"])
    assert np.array_equal(dis, g["dists"])


def test_cluster_fixtures_are_not_vacuous():
    """what make_hamming_golden.py asserts when it records, checked again on what is committed"""
    beyond = rerank = 0
    for p in glob.glob(os.path.join(GOLD, "clusters_*.npz")):
        g = np.load(p)
        k_walk, atleast = int(g["k_walk"]), int(g["atleast"])
        assert k_walk > 16
        tie = head = False
        for q in range(g["queries"].shape[0]):
            d = br.euclidean_no_sqrt(g["XQ"][q], g["centroids"])
            s = np.sort(d)
            assert (np.diff(s) > 1e-3 * s[1:]).all(), "two centre distances are close: the order would need a sort"
            cand = g["candidates"][q][:int(g["n_cand"][q])]
            rank = np.argsort(np.argsort(d))[g["clust_idx"][cand]]  # cluster after cluster in ascending centre distance,
            assert (np.diff(rank) >= 0).all() and (np.diff(cand)[np.diff(rank) == 0] > 0).all()  # rows ascending in each
            h = br.hamming_dists(g["rows"][cand], g["queries"][q:q + 1])[0]
            tie |= bool(cc.crosses(h, k_walk))
            head |= len(np.unique(h[:k_walk])) < k_walk
            if atleast > 1:
                beyond += len(cr.visited(g["centroids"], g["clust_idx"], g["XQ"][q], k_walk, 1)) < atleast
        assert tie and head, p
        if "factor" in g:
            rerank += 1
            for q in range(g["queries"].shape[0]):
                e = br.euclidean_no_sqrt(g["XQ"][q], g["X"][g["hamming_labels"][q]])
                assert e.max() <= 32767 and np.array_equal(e, np.round(e))
    assert beyond and rerank
