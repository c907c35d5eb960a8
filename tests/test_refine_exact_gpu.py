"""The resident refiner on the GPU (vaqhip_refiner_*, vaqhip_search_refine; vaq_amd/csrc/vaq_refine.hip) against
the fixtures recorded from the reference's VAQ::refine (tests/golden/refine/README.md) and against
tests/refine_ref.py, which test_refine_exact_cpu.py pins to those fixtures."""
import functools
import os
import subprocess

import numpy as np
import pytest

import refine_ref as rr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def run(refiner, Xq, cand, k, exact):
    refiner.exact_ties = exact
    ans = refiner.refine(Xq, cand, k)
    return ans.labels.reshape(len(Xq), k), ans.distances.reshape(len(Xq), k)


def check_both_rules(refiner, Xq, Xt, cand, k, id_base=0, what=""):
    """exact_ties on: the restatement of the reference slot for slot; off: the k smallest by (distance, label)"""
    for exact in (True, False):
        lab, dis = run(refiner, Xq, cand, k, exact)
        want_l, want_d = rr.refine(Xq, Xt, cand, k, exact=exact, id_base=id_base)
        assert bits_equal(dis, want_d), (what, exact)
        assert np.array_equal(lab, want_l), (what, exact)


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_goldens(vaqlib, name):
    """Every recorded answer: with exact_ties distances and labels slot for slot; without, the distances slot for slot
    and the labels after sorting each run of equal distances by label.  Where the k-th distance continues past the
    k-th slot the members of that last run are the heap's in the fixture and the smallest labels here (refine_ref.
    assert_default_rule); there the comparison with the restated (distance, label) rule is the exact one."""
    import vaq_amd
    c = rr.CASES[name]
    Xq, Xt, cand = rr.make_inputs(name)
    r = vaq_amd.VaqRefiner(c["D"])
    r.set_rows(Xt)
    d = rr.distances(Xq, Xt, cand)
    for k in c["ks"]:
        z = rr.load_fixture(name)
        want_l, want_d = z[f"labels_k{k}"], z[f"dists_k{k}"]
        lab, dis = run(r, Xq, cand, k, True)
        assert bits_equal(dis, want_d), (name, k)
        assert np.array_equal(lab, want_l), (name, k)
        lab, dis = run(r, Xq, cand, k, False)
        rr.assert_default_rule(lab, dis, want_l, want_d, what=f"{name} k={k}")
        sl = np.stack([rr.smallest_label_topk(d[q], cand[q], k)[0] for q in range(len(cand))])
        assert np.array_equal(lab, sl), (name, k)
    r.close()


@functools.lru_cache(maxsize=None)
def shape_rows():
    """N = 500 rows of 20 dims (one packet, a tail of 4 -- and a row is 80 bytes: candidate groups start at every
    alignment), built from 25 distinct vectors with a little noise so that equal and nearly equal distances occur."""
    rng = np.random.default_rng(77)
    base = rng.integers(0, 64, size=(25, 20)).astype(np.float32)
    Xt = base[rng.integers(0, 25, 500)]
    Xt[::3] += rng.uniform(-1e-3, 1e-3, size=Xt[::3].shape).astype(np.float32)
    Xq = rng.integers(0, 64, size=(65, 20)).astype(np.float32)
    return Xq, np.ascontiguousarray(Xt)


@pytest.fixture(scope="module")
def shape_refiner(vaqlib):
    import vaq_amd
    r = vaq_amd.VaqRefiner(20)
    r.set_rows(shape_rows()[1])
    yield r
    r.close()


@pytest.mark.parametrize("R", [1, 3, 16, 17, 200, 2048])
@pytest.mark.parametrize("nq", [1, 3, 65])
def test_shapes(shape_refiner, nq, R):
    """one query and more than a wave's worth; R below, at and just past the 16 candidate groups of a workgroup, no
    power of two, and the limit (candidates then repeat: N = 500); k = 1 and k = R"""
    Xq, Xt = shape_rows()
    rng = np.random.default_rng(1000 * nq + R)
    cand = rng.integers(0, 500, size=(nq, R)).astype(np.int32)
    for k in sorted({1, R}):
        check_both_rules(shape_refiner, Xq[:nq], Xt, cand, k, what=(nq, R, k))


def test_skipped_labels(vaqlib):
    """negative labels, labels below id_base and past the end, mixed into a list: skipped, the rest unchanged -- in
    the host form and in the device form, whose kernel checks every label itself"""
    import torch
    import vaq_amd
    Xq, Xt, cand = rr.make_inputs("cont_d40")
    k = 10
    r = vaq_amd.VaqRefiner(40)
    r.set_rows(Xt, id_base=1000)
    clean = cand + 1000
    mixed = np.insert(clean, [0, 5, 50, 200], [-7, 999, 1300, 2**31 - 1], axis=1).astype(np.int32)
    assert mixed.shape[1] == cand.shape[1] + 4
    for exact in (True, False):
        want_l, want_d = run(r, Xq, clean, k, exact)
        assert np.array_equal(want_l - 1000, rr.refine(Xq, Xt, cand, k, exact=exact)[0])
        lab, dis = run(r, Xq, mixed, k, exact)
        assert np.array_equal(lab, want_l) and bits_equal(dis, want_d), exact
        dl, dd = r.refine_device(torch.from_numpy(Xq).cuda(), torch.from_numpy(mixed).cuda(), k)
        torch.cuda.synchronize()
        assert np.array_equal(dl.cpu().numpy(), want_l) and bits_equal(dd.cpu().numpy(), want_d), exact
        # nothing admissible at all: every slot unfilled
        lab, dis = run(r, Xq, np.array([[-1, 5, 1300]] * len(Xq), np.int32), 2, exact)
        assert np.all(lab == -1) and np.all(dis == rr.FLT_MAX)
    r.close()


def test_id_base_and_add_rows(vaqlib):
    """labels are id_base + row; appended rows continue the numbering and can be refined at once"""
    import vaq_amd
    Xq, Xt, _ = rr.make_inputs("cont_d129")
    r = vaq_amd.VaqRefiner(129)
    r.set_rows(Xt[:120], id_base=1000)
    r.add_rows(Xt[120:250])
    r.add_rows(Xt[250:])
    rng = np.random.default_rng(9)
    cand = (1000 + np.stack([rng.permutation(np.arange(100, 300))[:64] for _ in range(len(Xq))])).astype(np.int32)
    assert (cand >= 1250).any() and (cand < 1120).any()
    check_both_rules(r, Xq, Xt, cand, 16, id_base=1000, what="appended")
    with pytest.raises(vaq_amd.VaqHipError) as e:
        r.set_rows(Xt, id_base=2**31 - 10)
    assert e.value.code == -6  # VAQHIP_ERANGE
    r.close()


def test_no_queries_and_limits(vaqlib):
    import vaq_amd
    r = vaq_amd.VaqRefiner(8)
    r.set_rows(np.zeros((4, 8), np.float32))
    ans = r.refine(np.empty((0, 8), np.float32), np.empty(0, np.int32), 3)
    assert ans.labels.size == 0 and ans.distances.size == 0
    import ctypes as C
    out_l, out_d = np.zeros(4, np.int32), np.zeros(4, np.float32)
    q = np.zeros((1, 8), np.float32)
    lin = np.zeros(4096, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert vaqlib.vaqhip_refiner_refine(r._h, p(q), 0, p(lin), 4, 2, p(out_l), p(out_d)) == 0  # nq = 0
    assert vaqlib.vaqhip_refiner_refine(r._h, p(q), 1, p(lin), 2049, 2, p(out_l), p(out_d)) == -2  # R > 2048
    assert vaqlib.vaqhip_refiner_refine(r._h, p(q), 1, p(lin), 4, 5, p(out_l), p(out_d)) == -2  # k > R
    assert vaqlib.vaqhip_refiner_refine(r._h, p(q), 1, p(lin), 4, 0, p(out_l), p(out_d)) == -1
    r.close()


def golden_index(name, exact):
    import vaq_amd
    z = np.load(os.path.join(GOLD, name + ".npz"))
    bits = [int(b) for b in z["bits"]]
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = [z[f"cent{s}"] for s in range(len(bits))]
    v.mEigenVectors = z["eig"]
    v.mCodebook = z["codes"]
    v.set_option("exact_ties", 1 if exact else 0)
    return v, z


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", ["d128_m8_b8", "d128_m32_b78"])
def test_fused_search_refine(vaqlib, oracle, name, exact):
    """search_refine(R = 100, k = 10) on a byte-code and a bit-packed golden index == search(100) + refiner.refine ==
    the restatement over the oracle's search result, with exact_ties on both objects and with it off"""
    import vaq_amd
    v, z = golden_index(name, exact)
    X = z["X"]
    N, D = z["codes"].shape[0], X.shape[1]
    base = (np.random.default_rng(5).uniform(-40, 40, size=(N, D))).astype(np.float32) + X[0]
    base[::7] = base[3]  # equal rows: equal refined distances
    r = vaq_amd.VaqRefiner(D)
    r.set_rows(base)
    r.exact_ties = exact
    fused = v.search_refine(X, 100, 10, r)
    cand = v.search(X, 100)
    two = r.refine(X, cand, 10)
    assert np.array_equal(fused.labels, two.labels) and bits_equal(fused.distances, two.distances)
    o_lab, _ = oracle.search(X, [z[f"cent{s}"] for s in range(len(z["bits"]))], z["codes"], 100, eig=z["eig"])
    if exact:
        assert np.array_equal(cand.labels.reshape(o_lab.shape), o_lab)
    want_l, want_d = rr.refine(X, base, o_lab, 10, exact=exact)
    assert np.array_equal(fused.labels.reshape(want_l.shape), want_l)
    assert bits_equal(fused.distances.reshape(want_d.shape), want_d)
    r.close()
    v.close()


def test_fused_refuses_other_rows(vaqlib):
    import vaq_amd
    v, z = golden_index("d128_m8_b8", False)
    N, D = z["codes"].shape[0], z["X"].shape[1]
    r = vaq_amd.VaqRefiner(D)
    r.set_rows(np.zeros((N - 1, D), np.float32))
    with pytest.raises(vaq_amd.VaqHipError) as e:
        v.search_refine(z["X"], 100, 10, r)
    assert e.value.code == -7  # VAQHIP_ESTATE: N differs
    r.set_rows(np.zeros((N, D), np.float32), id_base=3)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        v.search_refine(z["X"], 100, 10, r)
    assert e.value.code == -7  # id_base differs
    r.set_rows(np.zeros((N, D), np.float32))
    with pytest.raises(vaq_amd.VaqHipError) as e:
        v.search_refine(z["X"], 2048, 10, r)
    assert e.value.code == -2  # R > VAQHIP_MAX_K
    v.search_refine(z["X"], 100, 10, r)
    r.close()
    v.close()


def test_cpp_demo_refine_resident(vaqlib, oracle, tmp_path):
    """demo_vaqhip --refine 100,200 --refine-resident on a 20 000 x 128 float, non-integer base: the answer files
    are what the restatement predicts from the oracle's search result, label for label"""
    from helpers import make_case
    from vaq_amd import build, io
    exe = build.build_demo()
    c = make_case(612, 128, [8] * 8, 20000, 12, rotate=False)
    rng = np.random.default_rng(4)
    base = rng.uniform(0, 255, size=(20000, 128)).astype(np.float32)
    base[rng.integers(0, 20000, 4000)] = base[rng.integers(0, 20000, 4000)]  # equal rows among the candidates
    io.save_centroids(c["cents"], str(tmp_path / "c.bin"))
    io.save_codebook(c["codes"], str(tmp_path / "cb.bin"))
    io.write_vecs(str(tmp_path / "q.fvecs"), c["X"])
    io.write_vecs(str(tmp_path / "base.fvecs"), base)
    r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                        "--queries", str(tmp_path / "q.fvecs"), "--timeseries-size", "128", "--k", "100",
                        "--method", "VAQ64m8min8max8var1,HEAP", "--refine", "100,200", "--refine-resident",
                        "--exact-ties", "1", "--dataset-refine", str(tmp_path / "base.fvecs"),
                        "--result", str(tmp_path / "out.csv")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "Refine = 200 (resident rows, fused with the search)" in r.stdout and "20000 rows resident" in r.stdout
    for R in (100, 200):
        got = np.loadtxt(str(tmp_path / f"out.csv_R{R}"), delimiter=",", dtype=np.int64)
        cand, _ = oracle.search(c["X"], c["cents"], c["codes"], R)
        want_l, _ = rr.refine(c["X"], base, cand, 100)
        assert np.array_equal(got, want_l), R
