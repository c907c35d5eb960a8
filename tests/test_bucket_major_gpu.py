"""GPU parity of the bucket-major second pass (vaq_amd/csrc/vaq_scan_bm.hip; option
"bucket_major"): after a capped best-first pass every bucket still in some query's reach is
streamed once for all the queries that want it.  Checked against the CPU oracle
(VAQ::searchHeap's restatement) under the tie contract of helpers.assert_topk_matches, and
bit for bit against the library's own one-workgroup-per-query form: the result is the k
smallest (distance, label) pairs whatever order the rows are met in."""
import numpy as np
import pytest

from helpers import assert_topk_matches, make_case

pytestmark = pytest.mark.gpu


def make_index(c, bucket_bits=0):
    import vaq_amd
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(c["bits"])
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    if bucket_bits:
        v._ensure_index()
        v.set_option("bucket_bits", bucket_bits)
    v.mCodebook = c["codes"]
    return v


def oracle_all_dists(oracle, c, Xp):
    out = []
    for q in range(Xp.shape[0]):
        lut = oracle.create_lut(Xp[q], c["cents"], max(c["bits"]))
        out.append(oracle.all_dists(lut, c["codes"]))
    return np.stack(out)


def run(v, X, k, **opts):
    for key, val in opts.items():
        v.set_option(key, val)
    a = v.search(X, k)
    nq = X.shape[0]
    return a.labels.reshape(nq, k).copy(), a.distances.reshape(nq, k).copy(), v.last_timing()


CASES = [
    # seed, bits, N, nq, k, bucket_bits, make_case kwargs
    (9101, [8] * 16, 400_000, 96, 100, 0, {}),
    (9102, [8] * 8, 300_000, 70, 10, 0, {"dup_frac": 0.05}),
    (9103, [8] * 16, 300_000, 33, 100, 10, {"dup_frac": 0.02}),   # key continues into the second code
    (9104, [8] * 32, 260_000, 18, 37, 9, {}),                      # rows re-read in the tail (no carried words)
    (9105, [8] * 8, 500_000, 130, 1, 9, {}),
]


@pytest.mark.parametrize("seed,bits,N,nq,k,bb,kw", CASES, ids=[f"m{len(c[1])}_n{c[2] // 1000}k_k{c[4]}_b{c[5]}" for c in CASES])
def test_bucket_major_matches_oracle(vaqlib, oracle, seed, bits, N, nq, k, bb, kw):
    c = make_case(seed, 8 * len(bits) if len(bits) <= 16 else 4 * len(bits), bits, N, nq, **kw)
    c["X"][3] = np.nan  # a query without a valid table: all -1 (VAQ.cpp:1750: FLT_MAX > NaN is false)
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=8)
    ad = oracle_all_dists(oracle, c, Xp[:24])
    v = make_index(c, bb)
    v.set_option("timing", 1)
    base_l, base_d, t0 = run(v, c["X"], k, bucket_major=0)
    assert t0["bucket_major"] == 0
    assert_topk_matches(base_l[:24], base_d[:24], o_lab[:24], o_dis[:24], ad, what="one workgroup per query")
    seen = 0
    # (work units of a best-first first pass | 0 = sampled thresholds instead, candidate slots, queries per
    #  group, waves, buckets of the middle round)
    shapes = [(0, 0, 0, 0, 6), (0, 0, 4, 16, 0), (0, 8, 2, 8, 1), (0, 64, 4, 4, 3), (0, 1, 0, 0, 2),
              (1, 0, 4, 16, 0), (1, 0, 2, 8, 2), (4, 0, 4, 4, 6), (1, 8, 4, 16, 0), (2, 64, 2, 16, 1), (100000, 0, 0, 0, 0)]
    for units, cap, qb, nw, rnd in shapes:
        l, d, t = run(v, c["X"], k, bucket_major=2, bm_boot=0 if units else 2, bm_units=units, bm_candidates=cap,
                      bm_queries_per_group=qb, bm_waves=nw, bm_round=rnd)
        seen += t["bucket_major"]
        what = f"units={units} cap={cap} qb={qb} nw={nw} round={rnd}"
        assert np.array_equal(d.view(np.uint32), base_d.view(np.uint32)), what
        assert np.array_equal(l, base_l), what
        assert np.all(l[3] == -1)
    assert seen == len(shapes)
    # the order inside the buckets (rows of a bucket sorted by the second code; the pass skips whole
    # runs) is invisible: pass with the runs ignored, and an index built without that order
    for boot in (0, 2):
        l, d, t = run(v, c["X"], k, bucket_major=2, bm_boot=boot, bm_units=1, bm_candidates=0, bm_queries_per_group=0,
                      bm_waves=0, bm_runs=0, bm_round=6)
        assert t["bucket_major"] == 1 and np.array_equal(d.view(np.uint32), base_d.view(np.uint32)) and np.array_equal(l, base_l)
    v.set_option("bm_runs", 1)
    assert np.array_equal(base_d.view(np.uint32)[np.arange(nq) != 3], o_dis.view(np.uint32)[np.arange(nq) != 3])
    v.close()


def test_bucket_major_overflow_and_small_k(vaqlib, oracle):
    """Fewer than k rows within reach of pass A (k close to the rows of a bucket), candidate
    buffers of 1 slot (every query overflows and is finished by the best-first form).  N < k is
    tests/test_bucket_major_edges_gpu.py's (test_fewer_rows_than_k)."""
    bits = [8] * 8
    c = make_case(9201, 64, bits, 280_000, 40, dup_frac=0.3, integer=True)  # small integers: massive ties
    Xp = oracle.project(c["X"], c["eig"])
    for k in (256, 100):
        o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=8)
        v = make_index(c)
        v.set_option("timing", 1)
        base_l, base_d, _ = run(v, c["X"], k, bucket_major=0)
        for cap, boot in ((1, 0), (0, 0), (1, 2), (0, 2)):
            l, d, t = run(v, c["X"], k, bucket_major=2, bm_units=1, bm_candidates=cap, bm_boot=boot)
            assert t["bucket_major"] == 1
            assert np.array_equal(d.view(np.uint32), base_d.view(np.uint32)) and np.array_equal(l, base_l), (k, cap, boot)
        assert np.array_equal(base_d.view(np.uint32), o_dis.view(np.uint32))
        v.close()


def test_bucket_major_encoded_clustered(vaqlib, oracle):
    """Rows encoded from clustered SIFT-shaped vectors (real pruning: a query reaches a few per cent
    of the buckets), 1500 queries so that the automatic plan's shape is exercised: cost-ordered pass
    A, several groups per bucket, work stealing at the end."""
    import torch
    from vaq_amd import harness
    N, nq, k = 1_500_000, 1500, 100
    bits = [8] * 16
    base = harness.sift_like(N, 128, stream=0, device="cuda")
    Xq = harness.sift_like(nq, 128, stream=1, device="cuda")
    E = harness.pca_eigenvectors(base[:200_000])
    Ed = E.to("cuda")
    cents = harness.train_codebooks((base[:100_000] @ Ed), bits, iters=8)
    codes = harness.encode_torch(base @ Ed, cents).cpu().numpy().view(np.uint16)
    c = dict(bits=bits, cents=cents, eig=E.numpy(), codes=codes, X=Xq.cpu().numpy())
    del base
    torch.cuda.empty_cache()
    v = make_index(c, 10)
    v.set_option("timing", 1)
    base_l, base_d, t0 = run(v, c["X"], k, bucket_major=0)
    for boot in (2, 0, 1):
        l, d, t = run(v, c["X"], k, bucket_major=2, bm_boot=boot)
        assert t["bucket_major"] == 1 and t0["bucket_major"] == 0
        assert np.array_equal(d.view(np.uint32), base_d.view(np.uint32))
        assert np.array_equal(l, base_l)
    Xp = oracle.project(c["X"][:48], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=16)
    ad = oracle_all_dists(oracle, c, Xp)
    assert_topk_matches(l[:48], d[:48], o_lab, o_dis, ad, what="encoded, bucket-major")
    v.close()


def test_bucket_major_after_appends(vaqlib, oracle):
    """Rows appended in three pieces (vaqhip_index_add_codes_u16 merges them run by run, so the
    order inside the buckets survives), and an index built without that order: same results."""
    import vaq_amd
    bits = [8] * 16
    N, nq, k = 350_000, 64, 50
    c = make_case(9301, 128, bits, N, nq, dup_frac=0.03)
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=8)
    ad = oracle_all_dists(oracle, c, Xp[:16])
    res = {}
    for sub_order in (1, 0):
        v = vaq_amd.VaqHip()
        v.mBitsAlloc = list(bits)
        v.mCentroidsPerSubs = c["cents"]
        v.mEigenVectors = c["eig"]
        v._ensure_index()
        v.set_option("sub_order", sub_order)
        v.set_option("bucket_bits", 10)
        v.mCodebook = c["codes"][:250_000]
        v._ensure_codes()
        v.add_codes(c["codes"][250_000:340_000])
        v.add_codes(c["codes"][340_000:])
        v.set_option("timing", 1)
        for bm, boot in ((0, 0), (2, 0), (2, 2)):
            l, d, t = run(v, c["X"], k, bucket_major=bm, bm_units=1, bm_boot=boot)
            assert t["bucket_major"] == (1 if bm else 0)
            res[(sub_order, bm, boot)] = (l, d)
        v.close()
    base_l, base_d = res[(1, 0, 0)]
    assert_topk_matches(base_l[:16], base_d[:16], o_lab[:16], o_dis[:16], ad, what="appended")
    assert np.array_equal(base_d.view(np.uint32), o_dis.view(np.uint32))
    for key, (l, d) in res.items():
        assert np.array_equal(d.view(np.uint32), base_d.view(np.uint32)) and np.array_equal(l, base_l), key
