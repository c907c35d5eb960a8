"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle
on the same inputs and against the committed golden vectors.

Bar: LUT bit-exact; distances bit-exact; labels exact under the tie contract
(helpers.assert_topk_matches).  Distances are integer/IEEE-add work in a
defined order, so no tolerance is used; the only tolerance in this file is
for the un-ordered Eigen GEMM of ProjectOnEigenVectors, which is compared
with the oracle's fixed-order restatement bit-exactly and with float64 at
1e-4 relative (north_star)."""
import json
import os

import numpy as np
import pytest

from helpers import assert_topk_matches, make_case

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = sorted(json.load(open(os.path.join(GOLD, "manifest.json"))).keys())


def make_index(c, id_base=0):
    import vaq_amd
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(c["bits"])
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    v.id_base = id_base
    return v


def oracle_all_dists(oracle, c, Xp):
    out = []
    for q in range(Xp.shape[0]):
        lut = oracle.create_lut(Xp[q], c["cents"], max(c["bits"]))
        out.append(oracle.all_dists(lut, c["codes"]))
    return np.stack(out)


@pytest.mark.parametrize("name", CASES)
def test_golden(vaqlib, oracle, name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    bits = z["bits"].tolist()
    c = dict(bits=bits, cents=[z[f"cent{s}"] for s in range(len(bits))], eig=z["eig"],
             codes=z["codes"])
    v = make_index(c)
    Xp = v.project(z["X"])
    assert np.array_equal(Xp.view(np.uint32), z["Xproj"].view(np.uint32))
    lut = v.build_lut(z["X"])
    assert np.array_equal(lut.view(np.uint32), z["lut"].view(np.uint32))
    ad = oracle_all_dists(oracle, c, z["Xproj"])
    for key in z.files:
        if not key.startswith("labels_k"):
            continue
        k = int(key[len("labels_k"):])
        for qb, ea, bf in [(1, 1, 1), (1, 1, 0), (2, 1, 1), (4, 1, 1), (1, 0, 1), (2, 0, 1), (4, 0, 1), (1, 2, 1),
                           (2, 2, 1), (4, 2, 1), (2, 3, 1)]:
            v.set_option("queries_per_pass", qb)
            v.set_option("early_abandon", ea)
            v.set_option("best_first", bf)
            ans = v.search(z["X"], k)
            nq = z["X"].shape[0]
            assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k),
                                z[key], z[f"dists_k{k}"], ad, what=f"{name} k={k} qb={qb} ea={ea} bf={bf}")


CONFIGS = [
    # seed, D, bits, N, nq, k, kwargs
    (101, 128, [8] * 8, 20000, 9, 100, {}),
    (102, 128, [8] * 16, 20000, 5, 100, {"dup_frac": 0.05}),
    (103, 128, [8] * 32, 9000, 4, 100, {}),
    (104, 128, [12, 10, 9, 8, 8, 7, 6, 4], 20000, 6, 100, {}),
    (105, 64, [4] * 8, 30000, 7, 100, {}),            # 32-bit rows: one dword, heavy ties
    (106, 96, [5, 6, 7, 9, 11, 13, 3, 2, 1, 4, 8, 10], 8000, 3, 50, {}),  # fields straddle dwords
    (107, 16, [3] * 4, 5000, 16, 100, {"integer": True}),
    (108, 128, [8] * 8, 1000, 3, 1, {}),
    (109, 128, [8] * 8, 70000, 2, 1000, {}),           # k near the build's maximum
    (110, 128, [8] * 8, 20000, 33, 10, {"rotate": False}),
    (111, 32, [15, 1, 8, 8], 6000, 3, 20, {}),
    # the reference's default method string allows up to 13 bits in 32 subspaces: the lookup
    # tables (31488 floats; 126 KB per query) no longer fit LDS for 2+ queries per pass, so the
    # tail tables are read from global memory
    (112, 64, [13, 13, 12, 12, 11, 10] + [8] * 8 + [7] * 10 + [6] * 8, 8000, 4, 100, {}),
    (113, 48, [14, 14, 13, 13] + [6] * 8, 5000, 3, 64, {}),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[str(c[0]) for c in CONFIGS])
def test_search_matches_oracle(vaqlib, oracle, cfg):
    seed, D, bits, N, nq, k, kw = cfg
    c = make_case(seed, D, bits, N, nq, **kw)
    v = make_index(c)
    Xp = oracle.project(c["X"], c["eig"]) if c["eig"] is not None else c["X"]
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True)
    ad = oracle_all_dists(oracle, c, Xp)
    lut = v.build_lut(c["X"])
    o_lut = np.stack([oracle.create_lut(Xp[q], c["cents"], max(bits)) for q in range(nq)])
    assert np.array_equal(lut.view(np.uint32), o_lut.view(np.uint32))
    ties = 0
    bf_ran = 0
    for qb, slices, ea, hot, bf in [(1, 0, 1, 16, 1), (1, 0, 1, 16, 0), (2, 0, 1, 16, 1), (4, 0, 1, 32, 1),
                                    (2, 1, 1, 0, 1), (2, 3, 1, 5, 1), (1, 7, 1, 16, 0), (1, 7, 1, 16, 1),
                                    (1, 2, 1, 16, 1), (2, 0, 0, 16, 1), (4, 3, 0, 0, 1), (1, 1, 0, 16, 1),
                                    (2, 0, 2, 16, 1), (1, 5, 2, 32, 1), (4, 1, 2, 1, 1), (1, 1, 1, 32, 0),
                                    (1, 1, 1, 32, 1), (1, 1, 2, 0, 1)]:
        v.set_option("queries_per_pass", qb)
        v.set_option("slices", slices)
        v.set_option("early_abandon", ea)
        v.set_option("hot_buckets", hot)
        v.set_option("best_first", bf)
        v.set_option("timing", 1)
        ans = v.search(c["X"], k)
        bf_ran += v.last_timing()["best_first"]
        v.set_option("timing", 0)
        ties += assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), o_lab, o_dis,
                                    ad, what=f"cfg{seed} qb={qb} slices={slices} ea={ea} hot={hot} bf={bf}")
    if all(b == 8 for b in bits) and len(bits) in (8, 16, 32) and N >= 5000:
        assert bf_ran >= 3, bf_ran  # the best-first form has kernels for the byte layout
    if kw.get("integer"):
        assert ties > 0  # the boundary-tie rule was exercised


def test_projection_tolerance(vaqlib, oracle):
    c = make_case(201, 128, [8] * 8, 10, 64)
    v = make_index(c)
    Xp = v.project(c["X"])
    ref64 = c["X"].astype(np.float64) @ c["eig"].astype(np.float64)
    scale = np.abs(ref64).max()
    assert np.abs(Xp - ref64).max() <= 1e-4 * scale
    assert np.array_equal(Xp.view(np.uint32), oracle.project(c["X"], c["eig"]).view(np.uint32))


@pytest.mark.parametrize("D,bits", [(128, [8] * 16), (64, [8] * 8), (256, [8] * 32), (96, [8] * 8)], ids=["d128", "d64", "d256", "d96"])
def test_projection_many_rows_is_the_same_chain(vaqlib, oracle, D, bits):
    """From 65 536 rows on the projection runs tiled (a workgroup takes 16-64 rows, project_tile_kernel);
    every output is still one fmaf chain over the inner index ascending, so it equals the oracle's
    fixed-order product bit for bit -- ragged last tile, a NaN row, and D = 96 (no tiled kernel: the
    one-row-per-workgroup form)."""
    rng = np.random.default_rng(5)
    n = 65536 + 37
    c = make_case(209, D, bits, 10, 4)
    X = (rng.normal(size=(n, D)) * 30).astype(np.float32)
    X[7, 3] = np.nan
    v = make_index(c)
    got = v.project(X)
    want = oracle.project(X, c["eig"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the encoder on top of it: code for code
    X[7, 3] = 0.0
    v.encode(X, projected=False)
    want_codes = oracle.encode(oracle.project(X, c["eig"]), c["cents"], nthreads=8)
    assert np.array_equal(np.asarray(v.mCodebook), want_codes)


def test_edge_cases(vaqlib, oracle):
    import vaq_amd
    c = make_case(301, 32, [8] * 8, 50, 4)
    # empty database: every slot -1 / FLT_MAX (heap_reorder, utils/Heap.hpp:322-349)
    e = dict(c)
    e["codes"] = np.zeros((0, 8), np.uint16)
    v = make_index(e)
    ans = v.search(c["X"], 10)
    assert np.all(ans.labels == -1) and np.all(ans.distances == np.finfo(np.float32).max)
    # N < k: tail filled with -1 / FLT_MAX
    v = make_index(c)
    ans = v.search(c["X"], 100)
    lab = ans.labels.reshape(4, 100)
    o_lab, o_dis = oracle.search(c["X"], c["cents"], c["codes"], 100, eig=c["eig"])
    assert_topk_matches(lab, ans.distances.reshape(4, 100), o_lab, o_dis)
    assert np.all(lab[:, 50:] == -1)
    # zero queries
    ans = v.search(np.zeros((0, 32), np.float32), 5)
    assert ans.labels.size == 0
    # shard offset
    v2 = make_index(c, id_base=1000)
    a2 = v2.search(c["X"], 10)
    a1 = v.search(c["X"], 10)
    assert np.array_equal(a2.labels, a1.labels + 1000)
    v3 = make_index(c, id_base=2**31 - 10)
    with pytest.raises(vaq_amd.VaqHipError) as ei:
        v3.search(c["X"], 10)
    assert ei.value.code == -6
    # k above the build's limit
    with pytest.raises(vaq_amd.VaqHipError):
        v.search(c["X"], 5000)
    # NaN query: no row is ever admitted (CMax::cmp is false for NaN)
    Xn = c["X"].copy()
    Xn[0, 3] = np.nan
    ans = v.search(Xn, 5)
    assert np.all(ans.labels.reshape(4, 5)[0] == -1)
    o_lab, _ = oracle.search(Xn, c["cents"], c["codes"], 5, eig=c["eig"])
    assert np.array_equal(ans.labels.reshape(4, 5), o_lab)


def test_all_rows_identical(vaqlib, oracle):
    """Every row has the same code: all N distances are equal, the k
    smallest labels must come back (the reference keeps the first k it
    inserted, which are also rows 0..k-1)."""
    c = make_case(401, 32, [8] * 8, 20000, 3)
    c["codes"][:] = c["codes"][0]
    v = make_index(c)
    ans = v.search(c["X"], 100)
    lab = ans.labels.reshape(3, 100)
    assert np.array_equal(lab, np.tile(np.arange(100, dtype=np.int32), (3, 1)))
    o_lab, o_dis = oracle.search(c["X"], c["cents"], c["codes"], 100, eig=c["eig"])
    assert np.array_equal(np.sort(o_lab, 1), lab)
    assert np.array_equal(ans.distances.reshape(3, 100), o_dis)


def test_full_size_properties(vaqlib):
    """SIFT-1M shape (BASELINE configs[1]: N=1M, M=8 x 8 bit) through properties
    that do not need the oracle at full size: per-query results sorted,
    labels unique and in range, shard-and-merge of two halves == single index,
    and Qb = 1/2/4 agree bit for bit."""
    import torch
    import vaq_amd
    from vaq_amd.index import merge_topk_device
    c = make_case(501, 128, [8] * 8, 1_000_000, 64, dup_frac=0.01)
    v = make_index(c)
    k = 100
    res = {}
    for qb, ea, sl in [(1, 0, 0), (1, 1, 0), (2, 1, 0), (4, 1, 0), (2, 0, 5), (2, 1, 16), (4, 1, 61), (2, 2, 0), (1, 2, 33)]:
        v.set_option("queries_per_pass", qb)
        v.set_option("early_abandon", ea)
        v.set_option("slices", sl)
        v.set_option("hot_buckets", 0 if (qb, ea, sl) == (2, 1, 0) else 16)
        a = v.search(c["X"], k)
        res[(qb, ea, sl)] = (a.labels.reshape(64, k).copy(), a.distances.reshape(64, k).copy())
    v.set_option("slices", 0)
    v.set_option("early_abandon", 3)
    base = res[(1, 0, 0)]
    for key, r in res.items():
        assert np.array_equal(r[0], base[0]) and np.array_equal(r[1], base[1]), key
    lab, dis = base
    assert np.all(np.diff(dis, axis=1) >= 0)
    assert lab.min() >= 0 and lab.max() < 1_000_000
    assert all(len(set(r.tolist())) == k for r in lab)
    same = np.diff(dis, axis=1) == 0
    assert np.all(np.diff(lab, axis=1)[same] > 0)
    # two shards + merge == one index
    h = 500_000
    parts_l, parts_d = [], []
    for i, (a, b) in enumerate([(0, h), (h, 1_000_000)]):
        s = dict(c)
        s["codes"] = c["codes"][a:b]
        vs = make_index(s, id_base=a)
        q = torch.from_numpy(c["X"]).cuda()
        l, d = vs.search_device(q, k)
        parts_l.append(l)
        parts_d.append(d)
    torch.cuda.synchronize()
    ml, md = merge_topk_device(torch.stack(parts_d), torch.stack(parts_l), k)
    assert np.array_equal(ml.cpu().numpy(), lab) and np.array_equal(md.cpu().numpy(), dis)
    # the one-collective layout: [world, 2, nq, k] int32 (labels plane, distance-bits plane)
    from vaq_amd.index import merge_topk_packed_device
    packed = torch.stack([torch.stack([parts_l[i], parts_d[i].view(torch.int32)]) for i in range(2)]).contiguous()
    pl, pd = merge_topk_packed_device(packed, 2, 64, k)
    assert np.array_equal(pl.cpu().numpy(), lab) and np.array_equal(pd.cpu().numpy(), dis)


def test_cpp_demo_driver(vaqlib, oracle, tmp_path):
    """examples/demo_vaqhip.cpp (C++ adapter over the C ABI, index read from the
    reference's --save / --save-enc files) returns the oracle's neighbours."""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    c = make_case(601, 128, [8] * 8, 30000, 20, dup_frac=0.02)
    io.save_centroids(c["cents"], str(tmp_path / "c.bin"))
    io.save_codebook(c["codes"], str(tmp_path / "cb.bin"))
    c["eig"].astype(np.float32).tofile(str(tmp_path / "e.f32"))
    io.write_vecs(str(tmp_path / "q.fvecs"), c["X"])
    o_lab, o_dis = oracle.search(c["X"], c["cents"], c["codes"], 100, eig=c["eig"])
    io.write_vecs(str(tmp_path / "gt.ivecs"), o_lab.astype(np.int32))
    r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                        "--eigen", str(tmp_path / "e.f32"), "--queries", str(tmp_path / "q.fvecs"),
                        "--timeseries-size", "128", "--k", "100", "--method", "VAQ64m8min8max8var1,EA",
                        "--groundtruth", str(tmp_path / "gt.ivecs"), "--result", str(tmp_path / "out.csv")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.loadtxt(str(tmp_path / "out.csv"), delimiter=",", dtype=np.int64)
    Xp = oracle.project(c["X"], c["eig"])
    ad = np.stack([oracle.all_dists(oracle.create_lut(Xp[q], c["cents"], 8), c["codes"]) for q in range(20)])
    # distances are not in the CSV: check labels under the tie contract via their oracle distances
    d_got = np.take_along_axis(ad, got, axis=1).astype(np.float32)
    assert_topk_matches(got.astype(np.int32), d_got, o_lab, o_dis, ad, what="cpp demo")
    assert "precision(avg_recall): 1" in r.stdout


def test_cpp_demo_driver_refine_and_devices(vaqlib, oracle, tmp_path):
    """The rest of demo_vaq's query surface (demo_vaq.cpp:312-361, scripts/run_demos.sh "--refine
    100,200"): per R, search R candidates then VAQ::refine against the raw vectors -- here with
    the rows sharded over two logical devices (setDevices -> vaqhip_multi_search)."""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    c = make_case(611, 128, [8] * 8, 20000, 12)
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, size=(20000, 128)).astype(np.float32)  # the raw vectors refine() reads
    io.save_centroids(c["cents"], str(tmp_path / "c.bin"))
    io.save_codebook(c["codes"], str(tmp_path / "cb.bin"))
    c["eig"].astype(np.float32).tofile(str(tmp_path / "e.f32"))
    io.write_vecs(str(tmp_path / "q.fvecs"), c["X"])
    io.write_vecs(str(tmp_path / "base.fvecs"), base)
    r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                        "--eigen", str(tmp_path / "e.f32"), "--queries", str(tmp_path / "q.fvecs"),
                        "--timeseries-size", "128", "--k", "100", "--method", "VAQ64m8min8max8var1,HEAP",
                        "--refine", "100,200", "--dataset-refine", str(tmp_path / "base.fvecs"),
                        "--devices", "0,0", "--result", str(tmp_path / "out.csv")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "Refining the answer with Refine = 200" in r.stdout and "sharding the rows over 2" in r.stdout
    for R in (100, 200):
        got = np.loadtxt(str(tmp_path / f"out.csv_R{R}"), delimiter=",", dtype=np.int64)
        cand, _ = oracle.search(c["X"], c["cents"], c["codes"], R, eig=c["eig"])
        o_lab, o_dis = oracle.refine(c["X"], base, cand, 100)
        d_got = ((c["X"][:, None, :] - base[got]) ** 2).sum(-1).astype(np.float32)
        assert np.array_equal(np.sort(got, 1), np.sort(o_lab, 1)), R
        assert np.allclose(d_got, o_dis, rtol=1e-6), R


def test_run_demos_siftsmall_replay(vaqlib, oracle, tmp_path):
    """BASELINE configs[0] / scripts/run_demos.sh:5-22 replayed through demo_vaqhip with the script's own
    arguments: siftsmall shape (10 000 x 128 base, 100 queries), method VAQ256m32min7max8var1,HEAP,
    --k 100 --refine 100,200.  The base is synthetic (siftsmall_base.fvecs is not in the checkout) and
    the index comes from files, as training is out of scope: PCA + 32 codebooks of 256 from the harness,
    rows encoded by the product's encoder, saved in the reference's --save / --save-enc formats.
    Checked against oracle.search + oracle.refine for both refine values."""
    import subprocess
    import torch
    import vaq_amd
    from vaq_amd import build, harness, io
    exe = build.build_demo()
    N, nq, D, k = 10_000, 100, 128, 100
    bits = [8] * 32  # a 256-bit budget over 32 subspaces of 7..8 bits: every subspace gets 8
    base = harness.sift_like(N, D, stream=0, device="cuda")
    queries = harness.sift_like(nq, D, stream=1, device="cuda")
    E = harness.pca_eigenvectors(base)
    cents = harness.train_codebooks(base @ E.to("cuda"), bits, iters=10)
    v = vaq_amd.VaqHip()
    v.parseMethodString("VAQ256m32min7max8var1,HEAP")
    assert (v.mBitBudget, v.mSubspaceNum, v.mMinBitsPerSubs, v.mMaxBitsPerSubs) == (256, 32, 7, 8)
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = cents
    v.mEigenVectors = E.numpy()
    codes = v.encode_device(base, projected=False).cpu().numpy().view(np.uint16)
    v.close()
    base_h, q_h = base.cpu().numpy(), queries.cpu().numpy()
    del base, queries
    torch.cuda.empty_cache()
    io.save_centroids(cents, str(tmp_path / "c.bin"))
    io.save_codebook(codes, str(tmp_path / "cb.bin"))
    E.numpy().astype(np.float32).tofile(str(tmp_path / "e.f32"))
    io.write_vecs(str(tmp_path / "siftsmall_base.fvecs"), base_h)
    io.write_vecs(str(tmp_path / "siftsmall_query.fvecs"), q_h)
    gt = np.argsort(((q_h[:, None, :] - base_h[None, :, :]) ** 2).sum(-1), axis=1, kind="stable")[:, :k].astype(np.int32)
    io.write_vecs(str(tmp_path / "siftsmall_groundtruth.ivecs"), gt)
    method, refine = "VAQ256m32min7max8var1,HEAP", "100,200"
    result = str(tmp_path / f"answer_vaq_{method}_refine{refine}_sift_10K.csv")
    r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                        "--eigen", str(tmp_path / "e.f32"),
                        # scripts/run_demos.sh:11-22, argument for argument
                        "--dataset", str(tmp_path / "siftsmall_base.fvecs"),
                        "--queries", str(tmp_path / "siftsmall_query.fvecs"),
                        "--file-format-ori", "fvecs", "--timeseries-size", "128", "--dataset-size", "10000",
                        "--queries-size", "100", "--result", result,
                        "--groundtruth", str(tmp_path / "siftsmall_groundtruth.ivecs"), "--groundtruth-format", "ivecs",
                        "--method", method, "--k", "100", "--refine", refine],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "10000 rows x 32 subspaces" in r.stdout and "Refining the answer with Refine = 200" in r.stdout
    for R in (100, 200):
        got = np.loadtxt(result + f"_R{R}", delimiter=",", dtype=np.int64)
        assert got.shape == (nq, k)
        cand, _ = oracle.search(q_h, cents, codes, R, eig=E.numpy())
        o_lab, o_dis = oracle.refine(q_h, base_h, cand, k)
        d_got = ((q_h[:, None, :] - base_h[got]) ** 2).sum(-1).astype(np.float32)
        assert np.allclose(d_got, o_dis, rtol=1e-6), R
        # (integer-valued vectors: exact re-ranked distances tie; the candidate SETS must agree wherever
        #  the oracle's distances are distinct at the boundary)
        for qi in range(nq):
            inner = o_dis[qi] < o_dis[qi, -1]
            assert set(o_lab[qi][inner].tolist()) <= set(got[qi].tolist()), (R, qi)
    rec = [float(x.split(":")[1]) for x in r.stdout.splitlines() if "precision(avg_recall)" in x]
    assert len(rec) == 2 and rec[1] >= rec[0] > 0.5, rec  # refine 200 re-ranks a superset of refine 100's candidates


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[1], CONFIGS[4], CONFIGS[5], CONFIGS[6], CONFIGS[10]],
                         ids=lambda c: str(c[0]))
@pytest.mark.parametrize("bucket_bits", [1, 9, 10, 12])
def test_bucket_key_width(vaqlib, oracle, cfg, bucket_bits):
    """The bucketed row order keys on the top `bucket_bits` bits of the first code and, once
    that is used up, of the second (automatic only for >= 16M rows; forced here).  Results do
    not depend on it."""
    seed, D, bits, N, nq, k, kw = cfg
    c = make_case(seed, D, bits, N, nq, **kw)
    v = make_index(c)
    v._ensure_index()
    v.set_option("bucket_bits", bucket_bits)
    Xp = oracle.project(c["X"], c["eig"]) if c["eig"] is not None else c["X"]
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True)
    ad = oracle_all_dists(oracle, c, Xp)
    for qb, slices, ea, hot in [(1, 0, 1, 16), (2, 3, 1, 32), (4, 1, 2, 0), (2, 0, 2, 16), (1, 2, 0, 16)]:
        v.set_option("queries_per_pass", qb)
        v.set_option("slices", slices)
        v.set_option("early_abandon", ea)
        v.set_option("hot_buckets", hot)
        ans = v.search(c["X"], k)
        assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), o_lab, o_dis, ad,
                            what=f"cfg{seed} bucket_bits={bucket_bits} qb={qb} slices={slices} ea={ea} hot={hot}")


@pytest.mark.parametrize("bits", [[8] * 16, [12, 10, 9, 8, 8, 7, 6, 4]], ids=["m16", "nonuniform"])
def test_seeded_multislice(vaqlib, oracle, bits):
    """Few queries over many rows: rows are split over hundreds of workgroups,
    the sampling pre-pass seeds their thresholds and they exchange them through
    global memory.  Must equal the oracle and the unseeded / single-slice runs."""
    c = make_case(701, 128, bits, 2_400_000, 3, dup_frac=0.01)
    v = make_index(c)
    k = 100
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True, nthreads=3)
    ad = oracle_all_dists(oracle, c, Xp)
    seen = []
    for seed, slices, qb, ea, order in [(1, 300, 2, 1, 0), (0, 300, 2, 1, 0), (1, 0, 1, 3, 0), (1, 1, 2, 3, 0),
                                        (1, 257, 4, 2, 0), (1, 300, 2, 2, 0), (1, 300, 2, 1, 1), (1, 0, 1, 3, 1),
                                        (0, 2035, 2, 2, 1), (1, 77, 4, 1, 1)]:
        v.set_option("seed_thresholds", seed)
        v.set_option("early_abandon", ea)
        v.set_option("ordered_slices", order)
        v.set_option("slices", slices)
        v.set_option("queries_per_pass", qb)
        v.set_option("timing", 1)
        a = v.search(c["X"], k)
        t = v.last_timing()
        seen.append((seed, slices, t["slices"], t["seed_slices"]))
        assert_topk_matches(a.labels.reshape(3, k), a.distances.reshape(3, k), o_lab, o_dis, ad,
                            what=f"seed={seed} slices={slices} qb={qb} ea={ea} order={order}")
    assert seen[0][2] > 1 and seen[0][3] > 0, seen     # auto plan: multi-slice and seeded
    assert seen[1][3] == 0 and seen[3][3] == 0, seen   # seeding off / single slice


ENC_CASES = [
    # D, bits
    (128, [8] * 8),                       # L = 16
    (128, [8] * 16),                      # L = 8
    (128, [12, 10, 9, 8, 8, 7, 6, 4]),    # 4096 centroids stream through LDS in chunks
    (128, [8] * 32),                      # L = 4
    (128, [8] * 4),                       # L = 32
    (48, [5, 3, 2, 1]),                   # L = 12: generic path, tiny codebooks
    (8, [8] * 8),                         # L = 1
]


@pytest.mark.parametrize("D,bits", ENC_CASES, ids=[f"d{d}m{len(b)}" for d, b in ENC_CASES])
def test_encode_matches_oracle(vaqlib, oracle, D, bits):
    """VAQ::encode on the GPU == the oracle's restatement, code for code (same
    sequential summation order, strict <)."""
    c = make_case(801, D, bits, 10, 5)
    rng = np.random.default_rng(5)
    X = (rng.normal(size=(5000, D)) * 30).astype(np.float32)
    L = D // len(bits)
    if bits[0] >= 2:
        c["cents"][0][3] = c["cents"][0][2]      # two identical centroids: the first must win
    v = make_index(c)
    Xp = oracle.project(X, c["eig"])
    v.encode(X, projected=False)                  # GPU projection == oracle projection bit for bit
    assert np.array_equal(v.mCodebook, oracle.encode(Xp, c["cents"]))
    # plant (in PCA space) an exact copy of a centroid and an exact tie between two centroids
    Xp[0, :L] = c["cents"][0][1]
    Xp[1, :L] = c["cents"][0][2 if bits[0] >= 2 else 0]
    want = oracle.encode(Xp, c["cents"])
    v.encode(Xp, projected=True)
    assert np.array_equal(v.mCodebook, want)
    assert v.mCodebook[0, 0] == 1 and v.mCodebook[1, 0] == (2 if bits[0] >= 2 else 0)
    import torch
    got = v.encode_device(torch.from_numpy(Xp).cuda(), projected=True).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want)


def test_refine_matches_oracle(vaqlib, oracle):
    """vaqhip_refine against the oracle on integer-valued rows.  On integers every summation order gives
    the same bits, so this does not test the sequential-sum contract of include/vaqhip.h: continuous data,
    the edges of R and k and the device form are in tests/test_primitives_edges_gpu.py."""
    import vaq_amd
    rng = np.random.default_rng(9)
    N, D, nq, R, k = 5000, 128, 12, 200, 100
    Xt = rng.integers(0, 256, size=(N, D)).astype(np.float32)
    Xt[100] = Xt[7]                                # duplicate rows: exactly equal distances
    Xq = rng.integers(0, 256, size=(nq, D)).astype(np.float32)
    cand = np.stack([rng.permutation(N)[:R] for _ in range(nq)]).astype(np.int32)
    cand[0, :2] = [7, 100]
    o_lab, o_dis = oracle.refine(Xq, Xt, cand, k)
    v = vaq_amd.VaqHip()
    ans = v.refine(Xq, vaq_amd.LabelDistVec(cand.ravel(), np.zeros(cand.size, np.float32)), Xt, k)
    assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), o_lab, o_dis)
    # unfilled candidates (-1) are skipped
    cand2 = cand.copy()
    cand2[:, 150:] = -1
    ans2 = v.refine(Xq, vaq_amd.LabelDistVec(cand2.ravel(), np.zeros(cand.size, np.float32)), Xt, k)
    o2_lab, o2_dis = oracle.refine(Xq, Xt, cand[:, :150], k)
    assert_topk_matches(ans2.labels.reshape(nq, k), ans2.distances.reshape(nq, k), o2_lab, o2_dis)


def test_search_then_refine_pipeline(vaqlib, oracle):
    """demo_vaq.cpp:336-345: search with R candidates, refine to k against the
    raw vectors; the GPU pipeline equals the oracle pipeline."""
    import torch
    from vaq_amd import harness
    X = harness.sift_like(20000, 128, stream=1).numpy()
    Q = harness.sift_like(16, 128, stream=2).numpy()
    eig = harness.pca_eigenvectors(torch.from_numpy(X)).numpy()
    cents = harness.train_codebooks(torch.from_numpy(X @ eig), [8] * 8, iters=5)
    c = dict(bits=[8] * 8, cents=cents, eig=eig, codes=np.zeros((0, 8), np.uint16))
    v = make_index(c)
    v.encode(X, projected=False)
    assert np.array_equal(v.mCodebook, oracle.encode(oracle.project(X, eig), cents))
    ans = v.search(Q, 200)
    fin = v.refine(Q, ans, X, 100)
    o_l, o_d = oracle.search(Q, cents, v.mCodebook, 200, eig=eig)
    o_rl, o_rd = oracle.refine(Q, X, o_l, 100)
    assert_topk_matches(fin.labels.reshape(16, 100), fin.distances.reshape(16, 100), o_rl, o_rd)


@pytest.mark.parametrize("ndim,seed", [(10, 1), (3, 2), (37, 3), (64, 4)])
def test_query_lut_sequential(vaqlib, oracle, ndim, seed):
    """The reference's other entry on this path, BitVecEngine::queryLUT
    (BitVecEngine.hpp:1222-1343): one scalar quantiser per PCA dimension, columns
    summed one by one, any number of dimensions (not a multiple of 4)."""
    import vaq_amd
    rng = np.random.default_rng(seed)
    bits = rng.integers(1, 9, ndim).tolist() if ndim * 8 > 256 else rng.integers(1, 9, ndim).tolist()
    while sum(bits) > 256:
        bits[int(np.argmax(bits))] -= 1
    N, nq, k = 20000, 6, 50
    cent = np.zeros((256, ndim), np.float32)
    for d, b in enumerate(bits):
        cent[: 1 << b, d] = np.sort(rng.normal(size=1 << b) * 20).astype(np.float32)
    codes = np.stack([rng.integers(0, 1 << b, N) for b in bits], 1).astype(np.uint16)
    codes[N // 2:N // 2 + 500] = codes[:500]          # duplicates: exact ties
    q, _ = np.linalg.qr(rng.normal(size=(ndim, ndim)))
    eig = q.astype(np.float32)
    X = (rng.normal(size=(nq, ndim)) * 20).astype(np.float32)
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = [np.ascontiguousarray(cent[: 1 << b, d:d + 1]) for d, b in enumerate(bits)]
    v.mEigenVectors = eig
    v.mCodebook = codes
    Xp = oracle.project(X, eig)
    o_lab = np.empty((nq, k), np.int32)
    o_dis = np.empty((nq, k), np.float32)
    ad = np.empty((nq, N), np.float32)
    for i in range(nq):
        o_lab[i], o_dis[i] = oracle.query_lut_1d(Xp[i], bits, cent, codes, k)
        lut = [np.float32((Xp[i, d] - cent[: 1 << bits[d], d]) ** 2) for d in range(ndim)]
        acc = lut[0][codes[:, 0]].astype(np.float32)
        for d in range(1, ndim):
            acc = (acc + lut[d][codes[:, d]]).astype(np.float32)
        ad[i] = acc
    for qb, ea in [(1, 3), (2, 1), (4, 2), (1, 0), (2, 2)]:
        v.set_option("queries_per_pass", qb)
        v.set_option("early_abandon", ea)
        a = v.search(X, k)
        assert_topk_matches(a.labels.reshape(nq, k), a.distances.reshape(nq, k), o_lab, o_dis, ad,
                            what=f"queryLUT ndim={ndim} qb={qb} ea={ea}")


@pytest.mark.parametrize("with_eig", [True, False], ids=["rotated", "identity"])
def test_query_lut_checked_projection(vaqlib, oracle, with_eig):
    """BitVecEngine::queryLUT projects with checking (BitVecEngine.hpp:53-71 called at :1226): a PCA
    coordinate that comes out NaN or infinite becomes 0 before the tables are built.  One non-finite
    component of the query makes EVERY coordinate of z * V non-finite (NaN * 0 = NaN), so such a
    query is answered as the zero vector -- not with -1s, as VAQ::search (unchecked) answers."""
    import vaq_amd
    rng = np.random.default_rng(77)
    ndim, N, nq, k = 12, 5000, 6, 20
    bits = rng.integers(2, 9, ndim).tolist()
    cent = np.zeros((256, ndim), np.float32)
    for d, b in enumerate(bits):
        cent[: 1 << b, d] = np.sort(rng.normal(size=1 << b) * 20).astype(np.float32)
    codes = np.stack([rng.integers(0, 1 << b, N) for b in bits], 1).astype(np.uint16)
    eig = None
    if with_eig:
        q, _ = np.linalg.qr(rng.normal(size=(ndim, ndim)))
        eig = q.astype(np.float32)
    X = (rng.normal(size=(nq, ndim)) * 20).astype(np.float32)
    X[1, 3] = np.nan
    X[2, 0] = np.inf
    X[4, 5] = -np.inf
    X[4, 6] = np.nan
    # restatement of :53-71 on top of the oracle's fixed-order product (z * I for the identity)
    with np.errstate(invalid="ignore", over="ignore"):
        Xp = oracle.project(X, eig if with_eig else np.eye(ndim, dtype=np.float32))
    assert not np.isfinite(Xp[[1, 2, 4]]).any() and np.isfinite(Xp[[0, 3, 5]]).all()
    Xc = np.where(np.isfinite(Xp), Xp, np.float32(0)).astype(np.float32)
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = [np.ascontiguousarray(cent[: 1 << b, d:d + 1]) for d, b in enumerate(bits)]
    v.mEigenVectors = eig
    v.mCodebook = codes
    o_lab = np.empty((nq, k), np.int32)
    o_dis = np.empty((nq, k), np.float32)
    ad = np.empty((nq, N), np.float32)
    for i in range(nq):
        o_lab[i], o_dis[i] = oracle.query_lut_1d(Xc[i], bits, cent, codes, k)
        lut = [np.float32((Xc[i, d] - cent[: 1 << bits[d], d]) ** 2) for d in range(ndim)]
        acc = lut[0][codes[:, 0]].astype(np.float32)
        for d in range(1, ndim):
            acc = (acc + lut[d][codes[:, d]]).astype(np.float32)
        ad[i] = acc
    a = v.search(X, k)
    lab, dis = a.labels.reshape(nq, k), a.distances.reshape(nq, k)
    assert (lab >= 0).all()  # every query is answered
    assert_topk_matches(lab, dis, o_lab, o_dis, ad, what="queryLUT, checked projection")
    # VAQ::search does not check (VAQ.hpp:198-201): a NaN query has no row with heap_top > dist
    w = vaq_amd.VaqHip()
    w.mBitsAlloc = [4] * ndim
    w.mCentroidsPerSubs = [np.ascontiguousarray(cent[:16, d:d + 1]) for d in range(ndim)]
    w.mEigenVectors = eig
    w.mCodebook = (codes & 15).astype(np.uint16)
    b = w.search(X, k)
    assert (b.labels.reshape(nq, k)[1] == -1).all()


def test_lock_contention_stress(vaqlib, oracle):
    """Worst case for the workgroup admission lock: every row has the same code, so every
    row ties with the threshold distance and only the label order decides; 16 waves per
    workgroup, several slices, repeated runs must all return rows 0..k-1."""
    c = make_case(901, 128, [8] * 16, 400_000, 5)
    c["codes"][:] = c["codes"][7]
    v = make_index(c)
    v.set_option("waves_per_workgroup", 16)
    k = 100
    want = np.tile(np.arange(k, dtype=np.int32), (5, 1))
    for it, (qb, ea, sl, hot) in enumerate([(2, 1, 0, 16), (2, 1, 7, 16), (4, 1, 3, 0), (1, 2, 5, 16), (2, 0, 2, 16)] * 3):
        v.set_option("queries_per_pass", qb)
        v.set_option("early_abandon", ea)
        v.set_option("slices", sl)
        v.set_option("hot_buckets", hot)
        a = v.search(c["X"], k)
        assert np.array_equal(a.labels.reshape(5, k), want), (it, qb, ea, sl, hot)
    # and a tie-heavy but not degenerate case: 3-bit codes, 4096 distinct rows at most
    c2 = make_case(902, 16, [3] * 4, 200_000, 8, integer=True)
    v2 = make_index(c2)
    v2.set_option("waves_per_workgroup", 16)
    Xp = oracle.project(c2["X"], c2["eig"])
    o_lab, o_dis = oracle.search(Xp, c2["cents"], c2["codes"], k, max_bits=3, projected=True, nthreads=4)
    ad = oracle_all_dists(oracle, c2, Xp)
    for rep in range(4):
        v2.set_option("slices", [0, 3, 11, 1][rep])
        a = v2.search(c2["X"], k)
        assert_topk_matches(a.labels.reshape(8, k), a.distances.reshape(8, k), o_lab, o_dis, ad, what=f"ties rep {rep}")


def test_add_codes_appends_rows(vaqlib, oracle):
    """vaqhip_index_add_codes_u16: rows appended in three pieces (with an empty start and a TI
    regroup in between) give the same answers as one index over all of them."""
    from vaq_amd.index import NNMethod
    for bits, D in ([8] * 8, 64), ([12, 10, 9, 8, 8, 7, 6, 4], 64):
        c = make_case(801, D, bits, 30000, 8, dup_frac=0.02)
        full = c["codes"]
        v = make_index(dict(c, codes=full[:0]))
        Xp = oracle.project(c["X"], c["eig"])
        k = 50
        a = v.search(c["X"], k)
        assert np.all(a.labels == -1)
        v.add_codes(full[:7000])
        v.add_codes(full[7000:7001])
        v.add_codes(full[7001:])
        assert v.info()["N"] == 30000
        o_lab, o_dis = oracle.search(Xp, c["cents"], full, k, max_bits=max(bits), projected=True)
        ad = oracle_all_dists(oracle, dict(c, codes=full), Xp)
        a = v.search(c["X"], k)
        assert_topk_matches(a.labels.reshape(8, k), a.distances.reshape(8, k), o_lab, o_dis, ad, what="appended")
        v.close()
        # many small appends (merged into the bucketed order, never rebuilt) == one index, bit for bit
        rng = np.random.default_rng(4)
        cuts = np.sort(rng.choice(np.arange(12000, 30000), size=9, replace=False)).tolist() + [30000]
        w = make_index(dict(c, codes=full[:12000]))
        w.search(c["X"], k)
        lo = 12000
        for hi in cuts:
            w.add_codes(full[lo:hi])
            lo = hi
        ref = make_index(dict(c, codes=full)).search(c["X"], k)
        for slices in (0, 3):
            w.set_option("slices", slices)
            b = w.search(c["X"], k)
            assert np.array_equal(b.labels, ref.labels) and np.array_equal(b.distances, ref.distances), slices
        w.close()


@pytest.mark.parametrize("bits", [[8] * 12, [8] * 8, [12, 10, 9, 8, 8, 7, 6, 4]], ids=["m12", "m8", "nonuniform"])
def test_best_first_rounds_multislice(vaqlib, oracle, bits):
    """The best-first form where its rarely taken paths are the normal ones: thousands of tiny
    buckets (keys continued into the second code), more eligible buckets than one round holds,
    several slices per query whose workgroups adopt each other's thresholds in mid-setup (found
    by tools/fuzz_parity.py: a per-wave threshold made the workgroup-wide bisection diverge)."""
    c = make_case(9917, 4 * len(bits), bits, 4097, 33, dup_frac=0.05)
    k = 5
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True)
    ad = oracle_all_dists(oracle, c, Xp)
    ran = 0
    for bucket_bits in (8, 9, 10):
        v = make_index(c)
        v._ensure_index()
        v.set_option("bucket_bits", bucket_bits)
        for slices in (0, 2, 5):
            v.set_option("slices", slices)
            v.set_option("early_abandon", 1)
            v.set_option("waves_per_workgroup", 4)
            v.set_option("timing", 1)
            for rep in range(6):
                a = v.search(c["X"], k)
                assert_topk_matches(a.labels.reshape(33, k), a.distances.reshape(33, k), o_lab, o_dis, ad,
                                    what=f"bucket_bits={bucket_bits} slices={slices} rep={rep}")
            ran += v.last_timing()["best_first"]
        v.close()
    assert ran >= 4, ran


def test_two_streams_two_threads_one_index(vaqlib, oracle):
    """The index's workspaces are shared by every call: `_device` searches issued by two host
    threads on two different streams must not overwrite each other's lookup tables / partial
    lists (the library orders them with an event), and a host-buffer search in between must
    not either."""
    import threading
    import torch
    c = make_case(8801, 128, [8] * 8, 200_000, 64, dup_frac=0.01)
    v = make_index(c)
    k = 50
    X = torch.from_numpy(c["X"]).cuda()
    halves = [X[:32].contiguous(), X[32:].contiguous()]
    ref = [v.search(c["X"][:32], k), v.search(c["X"][32:], k)]
    errors = []

    def work(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for rep in range(40):
                    l, d = v.search_device(halves[i], k)
                    if rep % 8 == 0:  # a host-buffer call on the index's own stream in between
                        h = v.search(c["X"][i * 32:(i + 1) * 32], k)
                        assert np.array_equal(h.labels, ref[i].labels)
                    st.synchronize()
                    assert np.array_equal(l.cpu().numpy().ravel(), ref[i].labels), (i, rep)
                    assert np.array_equal(d.cpu().numpy().ravel(), ref[i].distances), (i, rep)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    # encode from two threads while searching (vaqhip_encode holds the index lock throughout)
    Xp = oracle.project(c["X"], c["eig"])
    o_codes = oracle.encode(Xp, c["cents"])

    def enc():
        try:
            for _ in range(10):
                import vaq_amd
                w = np.empty((64, 8), np.uint16)
                vaq_amd._lib.check(vaqlib.vaqhip_encode(v._h, Xp.ctypes.data, 64, 1, w.ctypes.data))
                assert np.array_equal(w, o_codes)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=enc), threading.Thread(target=work, args=(0,))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_boundary_ties_at_c2_size(vaqlib, oracle):
    """SIFT-1M shape (1M x 8 B, k = 100) with duplicates PLANTED at each query's k-th distance:
    several rows tie for the last places of the result.  The reference keeps whichever its heap
    happens to hold (utils/Heap.hpp:115-169); the contract here (DESIGN.md "Ties") is the
    smallest labels at that distance, distances bit-exact -- on both scan forms."""
    k, nq, N = 100, 8, 1_000_000
    c = make_case(7321, 128, [8] * 8, N, nq)
    Xp = oracle.project(c["X"], c["eig"])
    rng = np.random.default_rng(1)
    for q in range(nq):
        d = oracle.all_dists(oracle.create_lut(Xp[q], c["cents"], 8), c["codes"])
        kth = np.argpartition(d, k - 1)[k - 1]
        for dst in rng.integers(0, N, size=4):  # four more rows exactly as far away as the k-th best
            c["codes"][dst] = c["codes"][kth]
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=8)
    ad = oracle_all_dists(oracle, c, Xp)
    v = make_index(c)
    for bf in (1, 0):
        v.set_option("best_first", bf)
        a = v.search(c["X"], k)
        ties = assert_topk_matches(a.labels.reshape(nq, k), a.distances.reshape(nq, k), o_lab, o_dis, ad,
                                   what=f"planted ties bf={bf}")
        # every query has more rows at its k-th distance than places: the rule decided something
        assert sum(int((ad[q] == a.distances.reshape(nq, k)[q, -1]).sum() > 1) for q in range(nq)) == nq
        assert ties >= 1, ties


@pytest.mark.parametrize("bits", [[8] * 16, [12, 10, 9, 8, 8, 7, 6, 4], [8] * 8], ids=["m16", "nonuniform", "m8"])
def test_query_grouping_is_invisible(vaqlib, oracle, bits):
    """"group_queries": multi-query passes take the queries in the order of their nearest first
    and second codes; every result still lands in its own query's slot (ragged last pass,
    several slices with the pre-pass, in-place and queued forms)."""
    c = make_case(5150, 128, bits, 300_000, 37, dup_frac=0.02)
    v = make_index(c)
    k = 50
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True, nthreads=8)
    ad = oracle_all_dists(oracle, c, Xp)
    for qb, ea, slices, group in [(2, 1, 0, 2), (4, 1, 0, 2), (4, 2, 0, 2), (2, 1, 7, 2), (4, 1, 300, 2), (4, 0, 3, 2),
                                  (4, 1, 0, 0)]:
        v.set_option("queries_per_pass", qb)
        v.set_option("early_abandon", ea)
        v.set_option("slices", slices)
        v.set_option("group_queries", group)
        a = v.search(c["X"], k)
        assert_topk_matches(a.labels.reshape(37, k), a.distances.reshape(37, k), o_lab, o_dis, ad,
                            what=f"qb={qb} ea={ea} slices={slices} group={group}")
    a1 = v.search(c["X"][:1], k)  # fewer queries than a pass holds
    assert np.array_equal(a1.labels, a.labels[:k])


@pytest.mark.parametrize("k", [1, 37, 100, 160, 256, 300])
def test_best_first_pool_tie_cut(vaqlib, oracle, k):
    """The k-min pool of the best-first form when rows tying at the k-th distance fill it: the
    tie is cut by label (a bisection on the labels, vaq_scan_bf.h pool_compact).  4-bit codes in
    4 subspaces: at most 65 536 distinct rows among 300 000, so hundreds of rows share each
    distance; k from 1 to beyond the smallest pool (k = 300: 1024 slots, the LDS-resident
    bisection), with one and several slices per query."""
    c = make_case(4242 + k, 16, [4] * 4, 300_000, 6, integer=True)
    c["codes"][100_000:200_000] = c["codes"][:100_000]   # and every row at least twice
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=4, projected=True, nthreads=4)
    ad = oracle_all_dists(oracle, c, Xp)
    v = make_index(c)
    v.set_option("timing", 1)
    ran = 0
    for slices in (1, 0, 3):
        v.set_option("slices", slices)
        for nw in (4, 8):
            v.set_option("waves_per_workgroup", nw)
            a = v.search(c["X"], k)
            ran += v.last_timing()["best_first"]
            ties = assert_topk_matches(a.labels.reshape(6, k), a.distances.reshape(6, k), o_lab, o_dis, ad,
                                       what=f"k={k} slices={slices} nw={nw}")
            assert ties >= 1 or k == 1
    assert ran >= 2, ran
    v.close()


@pytest.mark.parametrize("bits,k", [([8] * 8, 100), ([8] * 16, 10), ([12, 10, 9, 8, 8, 7, 6, 4], 37), ([4] * 8, 100)],
                         ids=["m8", "m16", "nonuniform", "ties"])
def test_best_first_deferred_queries(vaqlib, oracle, bits, k):
    """Expensive queries cut in two ("defer_units"): a first round of a few work units, the buckets
    still in reach after it scanned by a second launch (two workgroups per query sharing a
    threshold) and merged into the first launch's result.  Forced with 1, 2 and 8 units, where
    nearly every query is handed over -- and more of them than the hand-over list holds, so some
    scan on in place -- against the oracle and against the undivided scan (bit-identical)."""
    N, nq = 200_000, 2500
    c = make_case(7100 + k, 4 * len(bits), bits, N, nq, dup_frac=0.02, integer=(bits[0] == 4))
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True, nthreads=8)
    v = make_index(c)
    v.set_option("timing", 1)
    v.set_option("defer_units", 0)
    base = v.search(c["X"], k)
    assert v.last_timing()["best_first"] == 1
    ad = oracle_all_dists(oracle, c, Xp[:64])
    assert_topk_matches(base.labels.reshape(nq, k)[:64], base.distances.reshape(nq, k)[:64], o_lab[:64], o_dis[:64], ad,
                        what="undivided")
    assert np.array_equal(base.distances.reshape(nq, k), o_dis)
    handed = {}
    for units in (1, 2, 8, -1):
        v.set_option("defer_units", units)
        for rep in range(2):
            a = v.search(c["X"], k)
            handed[units] = v.last_timing()["deferred_queries"]
            assert np.array_equal(a.distances, base.distances), (units, rep)
            assert np.array_equal(a.labels, base.labels), (units, rep)
    assert handed[1] == 2048, handed           # more expensive queries than the list holds
    assert handed[1] >= handed[2] >= handed[8] >= 1, handed
    assert handed[-1] == -1, handed            # the automatic rule: fewer than 4096 queries, not deferring
    v.close()


@pytest.mark.parametrize("bits", [[8] * 8, [12, 10, 9, 8, 8, 7, 6, 4], [4] * 8], ids=["m8", "nonuniform", "ties"])
def test_cost_ordered_dispatch_is_invisible(vaqlib, oracle, bits):
    """Expensive queries first ("cost_order", on by default from 1024 queries with one best-first
    workgroup per query): block b serves the b-th query of a ranking by how flat its first lookup
    table is.  Results land in the queries' own rows and are bit-identical with the ranking off."""
    N, nq, k = 150_000, 3000, 20
    c = make_case(8200 + len(bits), 4 * len(bits), bits, N, nq, dup_frac=0.02, integer=(bits[0] == 4))
    c["X"][7] = np.nan                      # a query without a valid table ranks last, and still gets its row
    c["X"][11] = c["X"][12]                 # identical queries: identical keys
    v = make_index(c)
    v.set_option("timing", 1)
    v.set_option("cost_order", 0)
    off = v.search(c["X"], k)
    assert v.last_timing()["best_first"] == 1 and v.last_timing()["slices"] == 1
    v.set_option("cost_order", 1)
    on = v.search(c["X"], k)
    assert np.array_equal(on.labels, off.labels) and np.array_equal(on.distances.view(np.uint32), off.distances.view(np.uint32))
    Xp = oracle.project(c["X"][:32], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True)
    ad = oracle_all_dists(oracle, c, Xp)
    good = [i for i in range(32) if i != 7]
    assert_topk_matches(on.labels.reshape(nq, k)[good], on.distances.reshape(nq, k)[good], o_lab[good], o_dis[good], ad[good],
                        what="ranked dispatch")
    # more queries than one internal launch takes (16384): every chunk is ranked on its own
    big = np.tile(c["X"], (6, 1))[:17000]
    v.set_option("timing", 0)
    on_big = v.search(big, k)
    v.set_option("cost_order", 0)
    off_big = v.search(big, k)
    assert np.array_equal(on_big.labels, off_big.labels)
    assert np.array_equal(on_big.distances.view(np.uint32), off_big.distances.view(np.uint32))
    sel = [i for i in range(3000) if i != 7]
    assert np.array_equal(on_big.labels.reshape(17000, k)[3000:6000][sel], on.labels.reshape(nq, k)[sel])
    v.close()
