"""The exhaustive form of the resident refiner on the GPU (vaqhip_refiner_search, vaq_amd.VaqRefiner.search): what
refine() would return for the candidate list id_base .. id_base + N - 1 in row order.  Labels and distance bit
patterns are compared with tests/refine_ref.py (pinned to the reference's fixtures by test_refine_exact_cpu.py) and,
where N <= 2048, with the merged refine kernel itself, with "exact_ties" on and off."""
import functools
import os
import subprocess

import numpy as np
import pytest

import refine_ref as rr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAX_K = 1024          # VAQHIP_MAX_K
ROW_TILE = 256        # vaq::XS_TILE: rows a workgroup takes at a time, one per thread
QUERY_TILE = 8        # XS_QB: queries between two barriers of the register form
MAX_DIM = 8176        # vaq::refine_rows_max_dim(): the widest row the refiner accepts
# N: the issue's sizes, one either side of the row tile (255, 257), and one either side of the split boundary at
# exhaustive_splits = 3 when every split is exactly one tile (767, 769)
SHAPE_N = [1, 9, 63, 64, 65, 255, 256, 257, 500, 767, 768, 769]
SHAPE_NQ = [1, 3, QUERY_TILE + 1, 65]
SHAPE_K = [1, 10, 100]
SPLITS = [0, 1, 3, 64]


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def all_rows(nq, N, id_base=0):
    return np.tile(np.arange(id_base, id_base + N, dtype=np.int32), (nq, 1))


def want(Xq, Xt, k, exact, id_base=0):
    with np.errstate(over="ignore", invalid="ignore"):  # (rows that overflow on purpose)
        return _want(Xq, Xt, k, exact, id_base)


def _want(Xq, Xt, k, exact, id_base):
    return rr.refine(Xq, Xt, all_rows(len(Xq), len(Xt), id_base), k, exact=exact, id_base=id_base)


def search(r, Xq, k, exact, splits=0):
    r.exact_ties = exact
    r.set_option("exhaustive_splits", splits)
    ans = r.search(Xq, k)
    return ans.labels.reshape(len(Xq), k), ans.distances.reshape(len(Xq), k)


def check(got, ref, what):
    assert bits_equal(got[1], ref[1]), what
    assert np.array_equal(got[0], ref[0]), what


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_fixture_inputs(vaqlib, name):
    """every path of Eigen's reduction (D = 7 .. 960, the last through the general path), the integer ties, and
    r2048's N = 3000 > 2048"""
    import vaq_amd
    c = rr.CASES[name]
    Xq, Xt, _ = rr.make_inputs(name)
    N = len(Xt)
    r = vaq_amd.VaqRefiner(c["D"])
    r.set_rows(Xt)
    for k in sorted({min(k, MAX_K) for k in c["ks"]}):
        for exact in (False, True):
            got = search(r, Xq, k, exact)
            check(got, want(Xq, Xt, k, exact), (name, k, exact))
            if N <= 2048 and k <= N:
                r.exact_ties = exact
                a = r.refine(Xq, all_rows(len(Xq), N), k)
                check(got, (a.labels.reshape(len(Xq), k), a.distances.reshape(len(Xq), k)), (name, k, exact, "refine"))
    r.close()


INT_KS = (1, 10, 100, 200)
INT_DRAW = 0  # the first draw on which every query ties across the k-th slot for every k of INT_KS (pinned by
              # test_exhaustive_cpu.py, as refine_ref.CASES["int_ties"] pins its own over 200 candidates)


@functools.lru_cache(maxsize=None)
def int_data(draw=INT_DRAW):
    """300 integer rows of 32 dims from 20 distinct vectors, 6 queries: every sum is exact, over ALL rows every
    query has a tie across the k-th slot, and the heap alone decides the labels"""
    rng = np.random.default_rng(4100 + draw)
    base = rng.integers(0, 256, size=(20, 32)).astype(np.float32)
    Xt = np.ascontiguousarray(base[rng.integers(0, 20, 300)])
    Xq = rng.integers(0, 256, size=(6, 32)).astype(np.float32)
    return Xq, Xt


def test_integer_rows_tied_at_every_k(vaqlib):
    import vaq_amd
    Xq, Xt = int_data()
    r = vaq_amd.VaqRefiner(32)
    r.set_rows(Xt)
    for k in INT_KS:
        for exact in (False, True):
            ref = want(Xq, Xt, k, exact)
            for S in SPLITS:
                check(search(r, Xq, k, exact, S), ref, (k, exact, S))
    r.close()


MIXED_K = 10


@functools.lru_cache(maxsize=None)
def mixed_data():
    """one batch with both outcomes of the flag step at k = MIXED_K: 200 continuous rows around the first four queries
    (no two equal distances among their first k + 1: copied out) and 200 copies of 10 integer vectors far away, around
    the last four (ties everywhere: replayed).  test_exhaustive_cpu.py keeps that true."""
    rng = np.random.default_rng(31)
    cont = rng.uniform(0, 255, size=(200, 20)).astype(np.float32)
    base = (rng.integers(0, 64, size=(10, 20)) + 1000).astype(np.float32)
    Xt = np.ascontiguousarray(np.concatenate([cont, base[rng.integers(0, 10, 200)]])[rng.permutation(400)])
    Xq = np.concatenate([rng.uniform(0, 255, size=(4, 20)), rng.integers(0, 64, size=(4, 20)) + 1000]).astype(np.float32)
    return Xq, Xt


def test_mixed_batch(vaqlib):
    """copied and replayed queries side by side; the replay count is the number of tied queries"""
    import vaq_amd
    Xq, Xt = mixed_data()
    r = vaq_amd.VaqRefiner(20)
    r.set_rows(Xt)
    r.set_option("timing", 1)
    for exact in (False, True):
        ref = want(Xq, Xt, MIXED_K, exact)
        for S in SPLITS:
            check(search(r, Xq, MIXED_K, exact, S), ref, (exact, S))
            assert r.last_search_timing()["listed_queries"] == (4 if exact else 0)
    r.close()


@functools.lru_cache(maxsize=None)
def shape_data():
    """rows of 20 dims (one packet and a tail of 4; a row is 80 bytes) built from 25 distinct vectors with a little
    noise on every third row: equal and nearly equal distances both occur -- shape_rows() of
    test_refine_exact_gpu.py, 769 rows long"""
    rng = np.random.default_rng(77)
    base = rng.integers(0, 64, size=(25, 20)).astype(np.float32)
    Xt = base[rng.integers(0, 25, max(SHAPE_N))]
    Xt[::3] += rng.uniform(-1e-3, 1e-3, size=Xt[::3].shape).astype(np.float32)
    Xq = rng.integers(0, 64, size=(max(SHAPE_NQ), 20)).astype(np.float32)
    return Xq, np.ascontiguousarray(Xt)


@functools.lru_cache(maxsize=None)
def shape_want(N, k, exact):
    Xq, Xt = shape_data()
    return want(Xq, Xt[:N], k, exact)


@pytest.mark.parametrize("N", SHAPE_N)
def test_shapes(vaqlib, N):
    """N around the row tile and the split boundary, nq around the query tile, k above and below N, every forced number
    of splits: one answer, the oracle's (the reference is computed once per (N, k, mode) for all 65 queries)"""
    import vaq_amd
    Xq, Xt = shape_data()
    r = vaq_amd.VaqRefiner(20)
    r.set_rows(Xt[:N])
    for k in SHAPE_K:
        for exact in (False, True):
            ref = shape_want(N, k, exact)
            for nq in SHAPE_NQ:
                for S in SPLITS:
                    got = search(r, Xq[:nq], k, exact, S)
                    check(got, (ref[0][:nq], ref[1][:nq]), (N, nq, k, exact, S))
    r.close()


def test_k_at_the_limit(vaqlib):
    """k = 1023 (a k + 1 list of 1024) and k = VAQHIP_MAX_K on 1500 integer rows, both tie modes"""
    import vaq_amd
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(40, 16)).astype(np.float32)
    Xt = np.ascontiguousarray(base[rng.integers(0, 40, 1500)])
    Xq = rng.integers(0, 256, size=(3, 16)).astype(np.float32)
    r = vaq_amd.VaqRefiner(16)
    r.set_rows(Xt)
    for k in (1023, 1024):
        for exact in (False, True):
            for S in (0, 3):
                check(search(r, Xq, k, exact, S), want(Xq, Xt, k, exact), (k, exact, S))
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        r.search(Xq, MAX_K + 1)
    assert e.value.code == -2
    r.close()


def test_id_base_and_appends(vaqlib):
    import vaq_amd
    Xq, Xt, _ = rr.make_inputs("int_ties")
    rng = np.random.default_rng(9)
    more = Xt[rng.integers(0, len(Xt), 41)]
    both = np.ascontiguousarray(np.concatenate([Xt, more]))
    r = vaq_amd.VaqRefiner(Xt.shape[1])
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        r.search(Xq, 10)
    assert e.value.code == -7  # no rows yet
    r.set_rows(Xt, id_base=1_000_000)
    for exact in (False, True):
        check(search(r, Xq, 10, exact), want(Xq, Xt, 10, exact, id_base=1_000_000), ("id_base", exact))
    r.add_rows(more)
    for exact in (False, True):
        for k in (10, 341, 400):
            got = search(r, Xq, k, exact)
            check(got, want(Xq, both, k, exact, id_base=1_000_000), ("append", k, exact))
            assert got[0].max() == 1_000_340 or k < 341
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        r.set_rows(Xt, id_base=2**31 - 100)
    assert e.value.code == -6
    r.close()


def test_rows_that_never_enter(vaqlib):
    """a row holding NaN and a row whose distance overflows to inf are never returned; with N - 2 < k the tail is
    -1 / FLT_MAX"""
    import vaq_amd
    rng = np.random.default_rng(21)
    Xt = rng.uniform(0, 255, size=(12, 20)).astype(np.float32)
    Xt[3, 17] = np.nan
    Xt[8, 2] = 3e38
    Xq = rng.uniform(0, 255, size=(4, 20)).astype(np.float32)
    Xq[:, 2] = -3e38
    Xt[[0, 1, 2, 4, 5, 6, 7, 9, 10, 11], 2] = -3e38
    r = vaq_amd.VaqRefiner(20)
    r.set_rows(Xt)
    for k in (5, 10, 12, 20):
        for exact in (False, True):
            lab, dis = search(r, Xq, k, exact)
            check((lab, dis), want(Xq, Xt, k, exact), (k, exact))
            assert not np.isin(lab, [3, 8]).any()
            if k > 10:
                assert np.all(lab[:, 10:] == -1) and np.all(dis[:, 10:] == rr.FLT_MAX)
                assert np.all(lab[:, :10] >= 0)
    r.close()


def test_search_device(vaqlib):
    """the _device form equals the host form; two calls back to back on one stream, the second larger (the workspace
    grows) and then the first again (it is reused), each against a fresh answer"""
    import torch
    import vaq_amd
    Xq, Xt = shape_data()
    r = vaq_amd.VaqRefiner(20)
    r.set_rows(torch.from_numpy(Xt).cuda())
    dq = torch.from_numpy(Xq).cuda()
    for exact in (False, True):
        r.exact_ties = exact
        r.set_option("exhaustive_splits", 0)
        a = r.search_device(dq[:3], 10)
        b = r.search_device(dq, 100)
        c = r.search_device(dq[:3], 10)
        torch.cuda.synchronize()
        for (l, d), nq, k in ((a, 3, 10), (b, 65, 100), (c, 3, 10)):
            ref = shape_want(len(Xt), k, exact)
            check((l.cpu().numpy(), d.cpu().numpy()), (ref[0][:nq], ref[1][:nq]), (exact, nq, k))
            h = r.search(Xq[:nq], k)
            check((l.cpu().numpy(), d.cpu().numpy()), (h.labels.reshape(nq, k), h.distances.reshape(nq, k)), "host form")
    r.close()


def test_wide_rows(vaqlib):
    """D = 129 (the first width past the register form) and the largest D the refiner accepts, N = 70"""
    import vaq_amd
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        vaq_amd.VaqRefiner(MAX_DIM + 1)
    assert e.value.code == -2
    for D in (129, MAX_DIM):
        rng = np.random.default_rng(D)
        base = rng.uniform(0, 255, size=(6, D)).astype(np.float32)
        Xt = (base[rng.integers(0, 6, 70)] + rng.uniform(-rr.NOISE, rr.NOISE, size=(70, D)).astype(np.float32)).astype(np.float32)
        Xt[40:] = np.round(Xt[40:])  # exact duplicates as well
        Xq = rng.uniform(0, 255, size=(3, D)).astype(np.float32)
        r = vaq_amd.VaqRefiner(D)
        r.set_rows(Xt)
        for k in (1, 10, 100):
            for exact in (False, True):
                for S in (0, 3):
                    check(search(r, Xq, k, exact, S), want(Xq, Xt, k, exact), (D, k, exact, S))
        r.close()


def test_timing_and_replay_count(vaqlib):
    """option "timing": on the integer rows every query has equal distances and is replayed; without exact_ties
    nothing is listed"""
    import vaq_amd
    Xq, Xt, _ = rr.make_inputs("int_ties")
    r = vaq_amd.VaqRefiner(Xt.shape[1])
    r.set_rows(Xt)
    r.set_option("timing", 1)
    search(r, Xq, 10, True, 3)
    t = r.last_search_timing()
    assert t["listed_queries"] == len(Xq) and t["splits"] == 3 and t["register_form"] == 1
    assert t["select_ms"] > 0 and t["replay_ms"] > 0
    search(r, Xq, 10, False)
    assert r.last_search_timing()["listed_queries"] == 0
    r.close()


def test_demo_exact_groundtruth(vaqlib, tmp_path):
    """demo_vaqhip --exact-groundtruth prints the recall it prints with a ground-truth file.  The queries are
    tests/golden/siftsmall/siftsmall_query.fvecs; siftsmall's base vectors are not in the checkout, so the base is
    the harness's SIFT-like one and the file holds ITS ground truth ((distance, label) order: integer-valued vectors,
    every float32 sum exact), as in test_parity_gpu.py's replay of run_demos.sh."""
    import torch
    import vaq_amd
    from vaq_amd import build, harness, io
    exe = build.build_demo()
    N, D, k = 10_000, 128, 100
    q_h = io.read_fvecs(os.path.join(GOLD, "siftsmall", "siftsmall_query.fvecs")).astype(np.float32)
    nq = len(q_h)
    bits = [8] * 8
    base = harness.sift_like(N, D, stream=0, device="cuda")
    E = harness.pca_eigenvectors(base)
    cents = harness.train_codebooks(base @ E.to("cuda"), bits, iters=4)
    v = vaq_amd.VaqHip()
    v.parseMethodString("VAQ64m8min8max8var1,HEAP")
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = cents
    v.mEigenVectors = E.numpy()
    codes = v.encode_device(base, projected=False).cpu().numpy().view(np.uint16)
    v.close()
    base_h = base.cpu().numpy()
    del base
    torch.cuda.empty_cache()
    io.save_centroids(cents, str(tmp_path / "c.bin"))
    io.save_codebook(codes, str(tmp_path / "cb.bin"))
    E.numpy().astype(np.float32).tofile(str(tmp_path / "e.f32"))
    io.write_vecs(str(tmp_path / "base.fvecs"), base_h)
    io.write_vecs(str(tmp_path / "q.fvecs"), q_h)
    d = ((q_h[:, None, :].astype(np.float64) - base_h[None, :, :]) ** 2).sum(-1)
    gt = np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)
    io.write_vecs(str(tmp_path / "gt.ivecs"), gt)
    common = [exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
              "--eigen", str(tmp_path / "e.f32"), "--dataset", str(tmp_path / "base.fvecs"),
              "--queries", str(tmp_path / "q.fvecs"), "--timeseries-size", "128", "--queries-size", str(nq),
              "--method", "VAQ64m8min8max8var1,HEAP", "--k", str(k)]
    outs = []
    for extra in (["--groundtruth", str(tmp_path / "gt.ivecs")], ["--exact-groundtruth"],
                  ["--exact-groundtruth", "--refine", "200", "--refine-resident"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        outs.append([x for x in r.stdout.splitlines() if "precision(avg_recall)" in x or "recall@R" in x])
    assert len(outs[0]) == 2 and outs[0] == outs[1], outs
    assert len(outs[2]) == 2 and float(outs[2][0].split(":")[1]) >= float(outs[0][0].split(":")[1]) > 0.1, outs
