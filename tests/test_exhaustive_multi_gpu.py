"""The exhaustive form across the shards of a multi-device refiner on the GPU (vaqhip_multi_refiner_search,
vaq_amd.VaqMultiRefiner.search): what vaqhip_refiner_search returns for the same rows, slot for slot, although the rows
are cut into shards.  Logical shards on device 0 exercise every step (select per shard, gather, merge, the flag step on
the merged lists, the chain of replays).  Labels are compared with array_equal and distances by bit pattern against
tests/refine_ref.py over all rows and, where stated, against VaqRefiner.search on the same rows.

test_exhaustive_multi_cpu.py asserts on the integer rows themselves that for G = 2, 3 and 8 every (query, k) has a run
of rows tied at the k-th distance that crosses a shard cut and slot k: a flag step or a replay per shard, merged
afterwards, fails test_integer_rows_tied_across_the_cuts."""
import functools
import os
import subprocess

import numpy as np
import pytest

import refine_ref as rr
from test_exhaustive_gpu import INT_KS, MIXED_K, MAX_K, check, int_data, mixed_data, shape_data, want

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def multi(G, D, Xt=None, id_base=0):
    import vaq_amd
    r = vaq_amd.VaqMultiRefiner([0] * G, D)
    if Xt is not None:
        r.set_rows(Xt, id_base=id_base)
    return r


def search(r, Xq, k, exact, splits=0):
    r.exact_ties = exact
    r.set_option("exhaustive_splits", splits)
    ans = r.search(Xq, k)
    return ans.labels.reshape(len(Xq), k), ans.distances.reshape(len(Xq), k)


@pytest.mark.parametrize("G", [2, 3, 8])
def test_integer_rows_tied_across_the_cuts(vaqlib, G):
    Xq, Xt = int_data()
    r = multi(G, 32, Xt)
    assert r.info()["shard_rows"][0] == -(-300 // G)
    for k in INT_KS:
        for exact in (False, True):
            ref = want(Xq, Xt, k, exact)
            for S in (0, 1, 3):
                check(search(r, Xq, k, exact, S), ref, (G, k, exact, S))
    r.close()


@pytest.mark.parametrize("G", [2, 3])
def test_mixed_batch(vaqlib, G):
    """copied and replayed queries side by side; the flag step on the merged lists lists exactly the tied queries"""
    Xq, Xt = mixed_data()
    r = multi(G, 20, Xt)
    r.set_option("timing", 1)
    for exact in (False, True):
        check(search(r, Xq, MIXED_K, exact), want(Xq, Xt, MIXED_K, exact), (G, exact))
        t = r.last_search_timing()
        assert t["listed_queries"] == (4 if exact else 0), t
        assert t["chain_shards"] == G and t["sets"] == 1, t
    r.close()


SHAPES = [(8, N) for N in (1, 2, 7, 8, 9)] + [(2, N) for N in (511, 512, 513)] + [(3, N) for N in (767, 768, 769)]
SHAPE_NQ = [1, 9, 65]
SHAPE_K = [1, 10, 100]


@functools.lru_cache(maxsize=None)
def shape_want(N, k, exact):
    Xq, Xt = shape_data()
    return want(Xq, Xt[:N], k, exact)


@pytest.mark.parametrize("G,N", SHAPES)
def test_shapes(vaqlib, G, N):
    """N around the cuts: empty shards, one row per shard and one more at G = 8; either side of the row tile per shard
    at G = 2 and 3; k above and below a shard's rows and above N (the reference is computed once per (N, k, mode))"""
    Xq, Xt = shape_data()
    r = multi(G, 20, Xt[:N])
    for k in SHAPE_K:
        for exact in (False, True):
            ref = shape_want(N, k, exact)
            for nq in SHAPE_NQ:
                check(search(r, Xq[:nq], k, exact), (ref[0][:nq], ref[1][:nq]), (G, N, nq, k, exact))
    r.close()


@pytest.mark.parametrize("first", [0, 1])
def test_appends(vaqlib, first):
    """set_rows of 0 or 1 rows, then add_rows of the rest: everything lands in the last shard (with first = 0 the
    first device holds no row and still merges); id_base = 1 000 000, k crossing the appended range"""
    import vaq_amd
    Xq, Xt, _ = rr.make_inputs("int_ties")
    Xt = np.ascontiguousarray(Xt)
    base = 1_000_000
    one = vaq_amd.VaqRefiner(Xt.shape[1])
    one.set_rows(Xt, id_base=base)
    r = vaq_amd.VaqMultiRefiner([0, 0, 0], Xt.shape[1])
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        r.search(Xq, 10)
    assert e.value.code == -7  # no rows yet
    r.set_rows(Xt[:first], id_base=base)
    r.add_rows(Xt[first:])
    assert r.info()["shard_rows"] == [first, 0, len(Xt) - first]
    for exact in (False, True):
        for k in (1, 10, len(Xt) - 1, len(Xt) + 20):
            got = search(r, Xq, k, exact)
            check(got, want(Xq, Xt, k, exact, id_base=base), (first, k, exact))
            one.exact_ties = exact
            a = one.search(Xq, k)
            check(got, (a.labels.reshape(len(Xq), k), a.distances.reshape(len(Xq), k)), (first, k, exact, "single"))
    r.close()
    one.close()


def test_rows_that_never_enter(vaqlib):
    """the NaN row and the row whose distance overflows to inf sit in different shards (G = 3, N = 12: rows 3 and 8);
    neither is returned, and with N - 2 < k the tail is -1 / FLT_MAX"""
    rng = np.random.default_rng(21)
    Xt = rng.uniform(0, 255, size=(12, 20)).astype(np.float32)
    Xt[3, 17] = np.nan
    Xt[8, 2] = 3e38
    Xq = rng.uniform(0, 255, size=(4, 20)).astype(np.float32)
    Xq[:, 2] = -3e38
    Xt[[0, 1, 2, 4, 5, 6, 7, 9, 10, 11], 2] = -3e38
    r = multi(3, 20, Xt)
    for k in (5, 10, 12, 20):
        for exact in (False, True):
            lab, dis = search(r, Xq, k, exact)
            check((lab, dis), want(Xq, Xt, k, exact), (k, exact))
            assert not np.isin(lab, [3, 8]).any()
            if k > 10:
                assert np.all(lab[:, 10:] == -1) and np.all(dis[:, 10:] == rr.FLT_MAX)
                assert np.all(lab[:, :10] >= 0)
    r.close()


def test_k_at_the_limit(vaqlib):
    """k = VAQHIP_MAX_K (lists of 1025 under exact_ties) on the 1500 integer rows of test_exhaustive_gpu.py, G = 3"""
    import vaq_amd
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(40, 16)).astype(np.float32)
    Xt = np.ascontiguousarray(base[rng.integers(0, 40, 1500)])
    Xq = rng.integers(0, 256, size=(3, 16)).astype(np.float32)
    r = multi(3, 16, Xt)
    for exact in (False, True):
        check(search(r, Xq, MAX_K, exact), want(Xq, Xt, MAX_K, exact), (MAX_K, exact))
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        r.search(Xq, MAX_K + 1)
    assert e.value.code == -2
    r.close()


def test_wide_rows(vaqlib):
    """D = 129 (the general path of the select kernel), N = 70, G = 2"""
    D = 129
    rng = np.random.default_rng(D)
    base = rng.uniform(0, 255, size=(6, D)).astype(np.float32)
    Xt = (base[rng.integers(0, 6, 70)] + rng.uniform(-rr.NOISE, rr.NOISE, size=(70, D)).astype(np.float32)).astype(np.float32)
    Xt[40:] = np.round(Xt[40:])  # exact duplicates as well
    Xq = rng.uniform(0, 255, size=(3, D)).astype(np.float32)
    r = multi(2, D, Xt)
    for k in (1, 10, 100):
        for exact in (False, True):
            check(search(r, Xq, k, exact), want(Xq, Xt, k, exact), (k, exact))
    r.close()


def test_search_device(vaqlib):
    """the _device form three times back to back on one stream with no synchronise between them: small, larger (every
    buffer grows behind the first call's event), small again; equal to the host form and to the oracle"""
    import torch
    Xq, Xt = shape_data()
    r = multi(3, 20, Xt)
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


def test_more_than_one_set(vaqlib):
    """nq = 16384 + 40 on 3 shards: the _device call is cut into equal sets (pointer offsets per set, the buffers of a
    set reused by the next), the host form into two staged calls.  The integer rows tiled: every query ties across the
    cuts (test_exhaustive_multi_cpu.py), so under exact_ties every query of every set is listed and replayed.  The
    expected answer is computed on the 6 distinct queries and tiled.

    The answers are checked WITHOUT option "timing" first: the sets of a _device call are then only enqueued, with no
    host synchronise between them, so the next set's reuse of the gathered lists, the merged lists, the replay list and
    the heap arrays rests on the stream waits alone; sets and chain_shards are reported without the option too.

    Under "timing" listed_queries is summed over the sets of one call like the times: after search_device it is the
    call's nq; after the host form, whose staged calls each start the figures anew, it is the last staged call's share
    of the queries, worked out from the set size info() reports."""
    import torch
    Xq, Xt = int_data()
    r = multi(3, 32, Xt)
    SET = r.info()["set_queries"]
    nq = SET + 40
    last = nq - (nq - 1) // SET * SET
    pick = np.arange(nq) % len(Xq)
    Xq_t = np.ascontiguousarray(Xq[pick])
    dq = torch.from_numpy(Xq_t).cuda()
    for timing in (0, 1):
        r.set_option("timing", timing)
        for exact in (False, True):
            for k in (1, 10):
                ref = want(Xq, Xt, k, exact)
                ref = (ref[0][pick], ref[1][pick])
                check(search(r, Xq_t, k, exact), ref, (timing, k, exact, "host form"))
                t = r.last_search_timing()
                assert t["chain_shards"] == 3 and t["sets"] == 1, t
                assert t["listed_queries"] == (last if exact and timing else 0), t
                l, d = r.search_device(dq, k)
                torch.cuda.synchronize()
                check((l.cpu().numpy(), d.cpu().numpy()), ref, (timing, k, exact, "device form"))
                t = r.last_search_timing()
                assert t["sets"] >= 2 and t["chain_shards"] == 3, t
                assert t["listed_queries"] == (nq if exact and timing else 0), t
    r.close()


def test_one_shard_is_the_single_form(vaqlib):
    import vaq_amd
    Xq, Xt = int_data()
    one = vaq_amd.VaqRefiner(32)
    one.set_rows(Xt)
    r = multi(1, 32, Xt)
    r.set_option("timing", 1)
    for exact in (False, True):
        for k in (10, 200):
            one.exact_ties = exact
            a = one.search(Xq, k)
            got = search(r, Xq, k, exact)
            check(got, (a.labels.reshape(len(Xq), k), a.distances.reshape(len(Xq), k)), (k, exact))
            check(got, want(Xq, Xt, k, exact), (k, exact, "oracle"))
            t = r.last_search_timing()
            assert t["listed_queries"] == (len(Xq) if exact else 0) and t["gather_ms"] == 0 and t["chain_ms"] == 0, t
    r.close()
    one.close()


def test_cpp_shim(vaqlib, tmp_path):
    """VaqHip::searchExhaustive after setDevices({0, 0}) and setRefineDataset equals the single-device object's answer,
    refineExactTies off and on (tests/cpp/exhaustive_multi_shim_test.cpp)"""
    from vaq_amd import build
    Xq, Xt = int_data()
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([len(Xt), Xt.shape[1], len(Xq), 100], np.int32).tobytes())
        f.write(Xt.tobytes())
        f.write(Xq.tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "exhaustive_multi_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "exhaustive_multi_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "exhaustive_multi_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_exact_groundtruth_devices(vaqlib, tmp_path):
    """demo_vaqhip --devices 0,0 --exact-groundtruth prints the recall lines of the --groundtruth file run, with and
    without --refine R --refine-resident: the recipe of test_exhaustive_gpu.py::test_demo_exact_groundtruth"""
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
              "--method", "VAQ64m8min8max8var1,HEAP", "--k", str(k), "--devices", "0,0"]
    outs = []
    for extra in (["--groundtruth", str(tmp_path / "gt.ivecs")], ["--exact-groundtruth"],
                  ["--exact-groundtruth", "--refine", "200", "--refine-resident"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        assert "sharding the rows over 2 device entries" in r.stdout
        outs.append([x for x in r.stdout.splitlines() if "precision(avg_recall)" in x or "recall@R" in x])
    assert len(outs[0]) == 2 and outs[0] == outs[1], outs
    assert len(outs[2]) == 2 and float(outs[2][0].split(":")[1]) >= float(outs[0][0].split(":")[1]) > 0.1, outs
