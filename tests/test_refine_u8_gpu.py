"""Byte rows in the resident refiner on the GPU (vaqhip_refiner_*_u8; the uint8 instantiations of vaq_refine.hip's
kernels): a refiner that keeps a bvecs dataset as bytes answers as the float refiner of the same build does over
X.astype(float32) -- labels and distance bit patterns, slot for slot, for any float query, because (float)uint8 is
exact and nothing after the load differs.  The float refiner is pinned to the reference by test_refine_exact_gpu.py;
the two fixtures whose rows are integers in [0, 256) (int_ties, r2048) pin the byte path to the reference's recorded
answers directly."""
import functools
import os

import numpy as np
import pytest

import refine_ref as rr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ESTATE = -7


def equal(a, b):
    """np.array_equal on labels and on distances.view(uint32)"""
    return np.array_equal(a.labels, b.labels) and np.array_equal(np.asarray(a.distances, np.float32).view(np.uint32),
                                                                 np.asarray(b.distances, np.float32).view(np.uint32))


def byte_rows(rng, N, D):
    """random bytes, 0 and 255 forced into every row (D == 1: one of them, alternating)"""
    X = rng.integers(0, 256, size=(N, D), dtype=np.uint8)
    if D == 1:
        X[::2, 0], X[1::2, 0] = 0, 255
        return X
    a = rng.integers(0, D, N)
    b = (a + 1 + rng.integers(0, D - 1, N)) % D
    X[np.arange(N), a] = 0
    X[np.arange(N), b] = 255
    assert ((X == 0).any(1) & (X == 255).any(1)).all()
    return X


def pair(D, X8, id_base=0):
    """(byte refiner, float refiner) over the same rows"""
    import vaq_amd
    r8, rf = vaq_amd.VaqRefiner(D), vaq_amd.VaqRefiner(D)
    r8.set_rows_u8(X8, id_base=id_base)
    rf.set_rows(X8.astype(np.float32), id_base=id_base)
    assert r8.elem_size == 1 and rf.elem_size == 4
    return r8, rf


def check_refine(r8, rf, Xq, cand, ks, what=""):
    for exact in (False, True):
        r8.exact_ties = rf.exact_ties = exact
        for k in ks:
            assert equal(r8.refine(Xq, cand, k), rf.refine(Xq, cand, k)), (what, k, exact)


@pytest.mark.parametrize("name", ["int_ties", "r2048"])
def test_goldens(vaqlib, name):
    """rows that are integers in [0, 256): cast to uint8 without loss, and with exact_ties the byte refiner returns the
    reference's recorded labels and distances slot for slot, for every k of the case"""
    import vaq_amd
    c = rr.CASES[name]
    Xq, Xt, cand = rr.make_inputs(name)
    X8 = Xt.astype(np.uint8)
    assert np.array_equal(X8.astype(np.float32), Xt)  # the cast is lossless
    r = vaq_amd.VaqRefiner(c["D"])
    r.set_rows_u8(X8)
    r.exact_ties = True
    z = rr.load_fixture(name)
    for k in c["ks"]:
        ans = r.refine(Xq, cand, k)
        assert np.array_equal(ans.labels.reshape(-1, k), z[f"labels_k{k}"]), (name, k)
        assert np.array_equal(ans.distances.reshape(-1, k).view(np.uint32), z[f"dists_k{k}"].view(np.uint32)), (name, k)
    r.close()


@pytest.mark.parametrize("D", [1, 7, 8, 12, 16, 40, 100, 128, 129, 960])
def test_packet_edges_float_queries(vaqlib, D):
    """every path of Eigen's reduction with continuous queries; D = 1, 7 and 129 put row bases at odd addresses"""
    rng = np.random.default_rng(100 + D)
    X8 = byte_rows(rng, 300, D)
    Xq = rng.uniform(0, 255, size=(4, D)).astype(np.float32)
    cand = np.stack([rng.permutation(300)[:200] for _ in range(4)]).astype(np.int32)
    r8, rf = pair(D, X8)
    check_refine(r8, rf, Xq, cand, (10, 100), what=D)
    r8.close(), rf.close()


def test_label_handling(vaqlib):
    """id_base = 1000; negative labels, labels below id_base and at or past id_base + N are skipped, duplicated
    candidates kept; N = 1"""
    rng = np.random.default_rng(7)
    D, N = 24, 300
    X8 = byte_rows(rng, N, D)
    X8[::5] = X8[3]  # equal rows: equal distances
    Xq = rng.uniform(0, 255, size=(4, D)).astype(np.float32)
    r8, rf = pair(D, X8, id_base=1000)
    cand = (1000 + rng.integers(0, 40, size=(4, 64))).astype(np.int32)  # 64 draws from 40 rows: duplicates
    assert all(len(set(row)) < 64 for row in cand)
    mixed = np.insert(cand, [0, 5, 30, 64], [-7, 999, 1300, 2**31 - 1], axis=1).astype(np.int32)
    mixed[:, 10] = 1299  # the last row
    mixed[:, 11] = 1000  # the first
    check_refine(r8, rf, Xq, mixed, (1, 16, 68), what="mixed")
    for exact in (False, True):  # the skipped labels change nothing
        r8.exact_ties = exact
        clean = np.delete(mixed, [0, 6, 32, 67], axis=1)
        assert not ((clean < 1000) | (clean >= 1300)).any()
        assert equal(r8.refine(Xq, mixed, 16), r8.refine(Xq, np.ascontiguousarray(clean), 16)), exact
        none = r8.refine(Xq, np.array([[-1, 5, 1300]] * 4, np.int32), 2)
        assert np.all(none.labels == -1) and np.all(none.distances == rr.FLT_MAX)
    r8.close(), rf.close()
    r8, rf = pair(D, X8[:1], id_base=1000)
    check_refine(r8, rf, Xq, np.array([[1000, 1001, 999, 1000]] * 4, np.int32), (1, 4), what="N=1")
    r8.close(), rf.close()


def test_growth(vaqlib):
    """set_rows_u8 of 300 rows, then add_rows_u8 of 1, 149 and 700 (the 700 reallocates: growth by half reaches 450):
    after each step the answers of a float refiner built the same way"""
    rng = np.random.default_rng(11)
    D = 20
    X8 = byte_rows(rng, 1150, D)
    Xq = rng.uniform(0, 255, size=(4, D)).astype(np.float32)
    r8, rf = pair(D, X8[:300], id_base=50)
    n = 300
    for step in (0, 1, 149, 700):
        r8.add_rows_u8(X8[n:n + step])
        rf.add_rows(X8[n:n + step].astype(np.float32))
        n += step
        cand = (50 + np.stack([rng.permutation(n)[:min(n, 256)] for _ in range(4)])).astype(np.int32)
        cand[:, 0], cand[:, 1] = 50 + n - 1, 50 + n  # the last row, and one past it
        check_refine(r8, rf, Xq, cand, (10,), what=n)
        r8.exact_ties = rf.exact_ties = True
        assert equal(r8.search(Xq, 10), rf.search(Xq, 10)), n
    assert n == 1150
    r8.close(), rf.close()


def test_type_rules(vaqlib):
    """nothing is converted silently: an append of the other type is ESTATE; a set of either type replaces rows and
    type; a refiner without rows takes either"""
    import vaq_amd
    rng = np.random.default_rng(13)
    D = 12
    X8 = byte_rows(rng, 40, D)
    Xf = X8.astype(np.float32)
    Xq = rng.uniform(0, 255, size=(3, D)).astype(np.float32)
    cand = np.tile(np.arange(40, dtype=np.int32), (3, 1))
    r = vaq_amd.VaqRefiner(D)
    assert r.elem_size == 4
    r.add_rows_u8(X8[:10])  # an empty refiner takes add_rows_u8
    assert r.elem_size == 1
    r.add_rows_u8(X8[10:])
    want = r.refine(Xq, cand, 5)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        r.add_rows(Xf[:3])
    assert e.value.code == ESTATE and r.elem_size == 1
    assert equal(r.refine(Xq, cand, 5), want)  # the refused call changed nothing
    r.set_rows(Xf)  # switches back
    assert r.elem_size == 4
    assert equal(r.refine(Xq, cand, 5), want)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        r.add_rows_u8(X8[:3])
    assert e.value.code == ESTATE and r.elem_size == 4
    r.set_rows_u8(X8)
    assert r.elem_size == 1 and equal(r.refine(Xq, cand, 5), want)
    r.set_rows_u8(X8[:0])  # N == 0 takes either type
    r.add_rows(Xf)
    assert r.elem_size == 4 and equal(r.refine(Xq, cand, 5), want)
    r.set_rows(X8)  # set_rows stays as it is: a uint8 array handed to it is widened
    assert r.elem_size == 4 and equal(r.refine(Xq, cand, 5), want)
    for bad in (Xf, X8[:, :5], X8[:, ::-1]):  # the adapter converts nothing either
        with pytest.raises(vaq_amd.VaqHipError):
            r.set_rows_u8(bad)
    r.close()


def test_torch_device_rows(vaqlib):
    """set_rows_u8 from a uint8 tensor on the refiner's device == the host form"""
    import torch
    import vaq_amd
    rng = np.random.default_rng(17)
    D = 100
    X8 = byte_rows(rng, 300, D)
    Xq = rng.uniform(0, 255, size=(4, D)).astype(np.float32)
    cand = np.stack([rng.permutation(300)[:200] for _ in range(4)]).astype(np.int32)
    host, dev = vaq_amd.VaqRefiner(D), vaq_amd.VaqRefiner(D)
    host.set_rows_u8(X8, id_base=5)
    t = torch.from_numpy(X8).cuda()
    dev.set_rows_u8(t, id_base=5)
    del t
    assert dev.elem_size == 1
    check_refine(dev, host, Xq, cand + 5, (10, 100), what="torch")
    with pytest.raises(vaq_amd.VaqHipError):
        dev.set_rows_u8(torch.from_numpy(X8.astype(np.float32)).cuda())
    host.close(), dev.close()


@functools.lru_cache(maxsize=None)
def golden_index_inputs():
    z = np.load(os.path.join(GOLD, "d128_m8_b8.npz"))
    N = z["codes"].shape[0]
    base = byte_rows(np.random.default_rng(5), N, 128)
    base[::7] = base[3]  # equal rows: equal refined distances
    return z, base


@pytest.mark.parametrize("exact", [False, True])
def test_fused_search_refine(vaqlib, exact):
    """VaqHip.search_refine with a byte refiner == search followed by refine on the float refiner (the d128_m8_b8 golden
    index, 5000 rows)"""
    import vaq_amd
    z, base = golden_index_inputs()
    bits = [int(b) for b in z["bits"]]
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = [z[f"cent{s}"] for s in range(len(bits))]
    v.mEigenVectors = z["eig"]
    v.mCodebook = z["codes"]
    v.set_option("exact_ties", 1 if exact else 0)
    r8, rf = pair(128, base)
    r8.exact_ties = rf.exact_ties = exact
    X = z["X"]
    fused = v.search_refine(X, 100, 10, r8)
    two = rf.refine(X, v.search(X, 100), 10)
    assert equal(fused, two)
    r8.close(), rf.close(), v.close()


def test_cpp_demo_bvecs(vaqlib, tmp_path):
    """demo_vaqhip --file-format-ori bvecs --refine 100 --refine-resident --exact-groundtruth: the raw vectors go to the
    device as bytes, and the answer file and the recall lines are those of the same run over the widened fvecs files"""
    import subprocess
    from helpers import make_case
    from vaq_amd import build, io
    exe = build.build_demo()
    N = 5000
    c = make_case(613, 128, [8] * 8, N, 12, rotate=False)
    rng = np.random.default_rng(4)
    base = byte_rows(rng, N, 128)
    base[rng.integers(0, N, 1000)] = base[rng.integers(0, N, 1000)]  # equal rows among the candidates
    q8 = rng.integers(0, 256, size=(12, 128), dtype=np.uint8)
    io.save_centroids(c["cents"], str(tmp_path / "c.bin"))
    io.save_codebook(c["codes"], str(tmp_path / "cb.bin"))
    for ext, cast in (("bvecs", lambda a: a), ("fvecs", lambda a: a.astype(np.float32))):
        io.write_vecs(str(tmp_path / f"q.{ext}"), cast(q8))
        io.write_vecs(str(tmp_path / f"base.{ext}"), cast(base))
    out = {}
    for ext in ("bvecs", "fvecs"):
        r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                            "--queries", str(tmp_path / f"q.{ext}"), "--timeseries-size", "128", "--k", "10",
                            "--method", "VAQ64m8min8max8var1,HEAP", "--refine", "100", "--refine-resident",
                            "--exact-ties", "1", "--exact-groundtruth", "--file-format-ori", ext,
                            "--dataset", str(tmp_path / f"base.{ext}"), "--result", str(tmp_path / f"out_{ext}.csv")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        assert ("5000 rows resident, as bytes" in r.stdout) == (ext == "bvecs"), r.stdout
        assert "Exact ground truth" in r.stdout and "5000 rows x 12 queries" in r.stdout
        out[ext] = (np.loadtxt(str(tmp_path / f"out_{ext}.csv"), delimiter=",", dtype=np.int64),
                    [ln for ln in r.stdout.splitlines() if "recall" in ln])
    assert np.array_equal(out["bvecs"][0], out["fvecs"][0])
    assert out["bvecs"][1] == out["fvecs"][1] and len(out["bvecs"][1]) == 2
