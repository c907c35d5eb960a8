"""Method FAST across the shards of a multi-device index (vaqhip_multi_*, VaqHipMulti) on ONE GPU: logical
shards on device 0, as tests/test_multi_gpu.py uses them.  Every comparison is np.array_equal on labels and
distances, against BOTH the NumPy checker over all rows (tests/fast_ref.py) and a single-index VaqHipFast on
the same data.  The rule itself is pinned without a GPU in tests/test_fast_multi_cpu.py."""
import os

import numpy as np
import pytest

import fast_multi_ref as fm
import fast_ref as fr
from helpers import make_case

pytestmark = pytest.mark.gpu

FAST, HEAP = 0x08, 0x80


def fast_index(c, off=None, sc=None, methods="FAST", id_base=0):
    import vaq_amd
    v = vaq_amd.VaqHipFast(device=0)
    v.parseMethodString(f"VAQ{sum(c['bits'])}m{c['M']}min1max{max(c['bits'])}var1,{methods}")
    v.mBitsAlloc = c["bits"]
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    v.id_base = id_base
    if off is not None:
        v.setLUTQuantization(off, sc)
    return v


def spread_quant(lut, frac=0.9):
    """offsets / scales that spread every column over [0, 255 * frac]"""
    lo = lut.min(axis=(0, 2)).astype(np.float32)
    hi = lut.max(axis=(0, 2)).astype(np.float32)
    sc = (np.float32(255 * frac) / np.maximum(hi - lo, np.float32(1e-3))).astype(np.float32)
    return lo, sc


def multi(c, G, off, sc, id_base=0, codes=None, method=FAST):
    from vaq_amd.index import VaqHipMulti
    m = VaqHipMulti([0] * G, c["bits"], c["cents"], c["eig"])
    m.set_lut_quantization(off, sc)  # the quantisation first: without one the multi index refuses FAST
    m.set_method(method)
    m.set_codes(c["codes"] if codes is None else codes, id_base)
    return m


def same(ans, lab, dis, what=""):
    k = lab.shape[1]
    assert np.array_equal(ans.distances.reshape(-1, k), dis), what
    assert np.array_equal(ans.labels.reshape(-1, k), lab.astype(np.int32)), what


def check_all(c, Gs, ks, off, sc, id_base=0, what=""):
    """single index == checker, and every G == both"""
    v = fast_index(c, off, sc, id_base=id_base)
    lut = v.build_lut(c["X"])
    ms = {G: multi(c, G, off, sc, id_base=id_base) for G in Gs}
    for k in ks:
        el, ed = fr.search_fast(lut, off, sc, c["codes"], k, id_base=id_base)
        s = v.search(c["X"], k)
        same(s, el, ed, f"{what} single k={k}")
        for G, m in ms.items():
            a = m.search(c["X"], k)
            same(a, el, ed, f"{what} G={G} k={k}")
            assert np.array_equal(a.labels, s.labels) and np.array_equal(a.distances, s.distances)
    for m in ms.values():
        m.close()
    v.close()


def quant_for(c, frac=0.9):
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    v.close()
    return spread_quant(lut, frac)


@pytest.mark.parametrize("bits,D", [([4] * 8, 32), ([4] * 16, 64), ([4] * 64, 128), ([4, 4, 3, 3, 2, 2, 1, 1], 32),
                                    ([2] * 128, 128)], ids=["m8", "m16", "m64", "mixed", "m128x2"])
def test_shards_equal_single_index_and_checker(vaqlib, bits, D):
    """N = 20 000: the head lies in shard 0 for every G"""
    c = make_case(7000 + len(bits), D, bits, 20_000, 12, dup_frac=0.05)
    off, sc = quant_for(c)
    check_all(c, (1, 2, 3, 8), (1, 10, 100, 1024), off, sc, what=f"M={len(bits)}")


@pytest.mark.parametrize("N,G,k,spans", [(100, 8, 64, 5), (50, 3, 64, 3), (5, 8, 10, 5), (1, 3, 4, 1), (2000, 8, 1024, 5)])
def test_head_spanning_shards_and_empty_shards(vaqlib, N, G, k, spans):
    """the head (first min(k, N) rows) is spread over several shards; N < k; N < G leaves shards without rows"""
    bounds = fm.shard_bounds(N, G)
    kk = min(k, N)
    assert sum(1 for lo, hi in bounds if min(hi, kk) > min(lo, kk)) == spans
    c = make_case(7100 + N, 32, [4] * 8, N, 16, dup_frac=0.1)
    off, sc = quant_for(c, 0.2)  # few levels: ties inside the head and at the cut
    check_all(c, (G,), (k,), off, sc, id_base=12345, what=f"N={N} G={G}")


def test_saturated_tables_return_the_head_permutation(vaqlib):
    """every table entry 255: all distances tie at 255 M and the answer is std::sort's permutation of the head"""
    c = make_case(7200, 32, [4] * 8, 5000, 6)
    off, sc = np.full(8, -1e6, np.float32), np.full(8, 1e6, np.float32)
    v = fast_index(c, off, sc)
    assert int(v.buildSmallLUT(c["X"])[:, :, :16].min()) == 255
    v.close()
    check_all(c, (2, 3, 8), (17, 100, 1024), off, sc, what="saturated")
    m = multi(c, 3, off, sc)
    a = m.search(c["X"][:1], 100)
    assert np.array_equal(a.labels, fr.std_sort_perm(np.full(100, 255 * 8)).astype(np.int32))
    m.close()


def test_planted_duplicates_of_the_kth_distance(vaqlib):
    """rows carrying query 0's k-th distance on both sides of row k and on both sides of the shard boundary"""
    N, G, k = 20_000, 2, 100
    c = make_case(7300, 64, [4] * 16, N, 8)
    off, sc = quant_for(c)
    v = fast_index(c, off, sc)
    lut = v.build_lut(c["X"])
    v.close()
    d0 = fr.row_dists(fr.small_quantize(lut[0], off, sc), c["codes"])
    tau = np.sort(d0)[k - 1]
    src = int(np.nonzero(d0 == tau)[0][0])
    cut = fm.shard_bounds(N, G)[0][1]
    planted = [k - 3, k - 2, k - 1, k, k + 1, k + 2, cut - 2, cut - 1, cut, cut + 1]
    c["codes"][planted] = c["codes"][src]
    d0 = fr.row_dists(fr.small_quantize(lut[0], off, sc), c["codes"])
    assert np.sort(d0)[k - 1] == tau and int(np.sum(d0 == tau)) >= len(planted)   # still the k-th, now a wide tie
    assert int(np.sum(d0 <= tau)) > k                                                # and the cut goes through it
    check_all(c, (2, 3), (k, k + 1, 17), off, sc, what="planted")


def test_appends_extend_the_last_shard_and_may_grow_the_head(vaqlib):
    c = make_case(7400, 32, [4] * 8, 6000, 10, dup_frac=0.05)
    off, sc = quant_for(c, 0.3)
    v = fast_index(c, off, sc)
    lut = v.build_lut(c["X"])
    k, G = 64, 3
    m = multi(c, G, off, sc, id_base=500, codes=c["codes"][:40])
    for n0, n1 in ((0, 40), (40, 50), (50, 6000)):  # N < k; the head grows 40 -> 50; then past k
        if n0:
            m.add_codes(c["codes"][n0:n1])
        assert m.info()["N"] == n1 and m.info()["shard_rows"][-1] == n1 - 28
        cur = dict(c, codes=c["codes"][:n1])
        s = fast_index(cur, off, sc, id_base=500)
        for kq in (k, 17):
            el, ed = fr.search_fast(lut, off, sc, cur["codes"], kq, id_base=500)
            same(m.search(c["X"], kq), el, ed, f"after {n1} rows, multi")
            same(s.search(c["X"], kq), el, ed, f"after {n1} rows, single")
        s.close()
    m.close()
    v.close()


@pytest.mark.parametrize("nq", [1, 63, 65])
def test_query_counts(vaqlib, nq):
    c = make_case(7500 + nq, 64, [4] * 16, 9000, nq, dup_frac=0.05)
    off, sc = quant_for(c)
    check_all(c, (3,), (10,), off, sc, what=f"nq={nq}")


def test_queries_past_one_shards_chunk(vaqlib):
    """4M rows on two shards: a shard's chunk holds 2^29 / 2M = 256 queries, so 260 queries take two chunks on
    every shard (and three on the single index); all queries against the single index, both sides of the cut
    against the checker"""
    nq, k = 260, 20
    c = make_case(7600, 32, [4] * 8, 1 << 22, nq, rotate=False)
    off, sc = quant_for(c)
    v = fast_index(c, off, sc)
    lut = v.build_lut(c["X"])
    s = v.search(c["X"], k)
    m = multi(c, 2, off, sc)
    a = m.search(c["X"], k)
    assert np.array_equal(a.labels, s.labels) and np.array_equal(a.distances, s.distances)
    lab, dis = a.labels.reshape(nq, k), a.distances.reshape(nq, k)
    for q in (0, 255, 256, 259):
        el, ed = fr.search_fast(lut[q:q + 1], off, sc, c["codes"], k)
        assert np.array_equal(dis[q], ed[0]) and np.array_equal(lab[q], el[0].astype(np.int32)), q
    m.close()
    v.close()


def test_device_entry_with_torch_tensors(vaqlib):
    """vaqhip_multi_search_device: enqueue only, several searches back to back, one synchronisation; the
    caller's current device is left as it was"""
    import torch
    c = make_case(7700, 64, [4] * 16, 30_000, 33, dup_frac=0.05)
    off, sc = quant_for(c)
    v = fast_index(c, off, sc)
    m = multi(c, 3, off, sc)
    outs = []
    for n, k in ((33, 100), (5, 10), (33, 100), (17, 1)):
        q = torch.from_numpy(c["X"][:n]).cuda()
        outs.append((n, k, m.search_device(q, k)))
    assert torch.cuda.current_device() == 0
    torch.cuda.synchronize()
    lut = v.build_lut(c["X"])
    for n, k, (l, d) in outs:
        r = v.search(c["X"][:n], k)
        assert np.array_equal(l.cpu().numpy().ravel(), r.labels) and np.array_equal(d.cpu().numpy().ravel(), r.distances)
        el, ed = fr.search_fast(lut[:n], off, sc, c["codes"], k)
        assert np.array_equal(l.cpu().numpy(), el.astype(np.int32)) and np.array_equal(d.cpu().numpy(), ed)
    m.close()
    v.close()


def test_rccl_exchange_with_one_rank(vaqlib):
    """exchange = 1 on one shard runs the collective around the single-index FAST search"""
    c = make_case(7800, 32, [4] * 8, 20_000, 7)
    off, sc = quant_for(c)
    m = multi(c, 1, off, sc)
    m.set_option("exchange", 1)
    v = fast_index(c, off, sc)
    lut = v.build_lut(c["X"])
    el, ed = fr.search_fast(lut, off, sc, c["codes"], 50)
    a = m.search(c["X"], 50)
    assert m.info()["exchange"] == 1
    same(a, el, ed, "one rank, RCCL")
    same(v.search(c["X"], 50), el, ed, "single")
    m.close()
    v.close()


def test_fast_heap_fast_and_exact_ties(vaqlib):
    """FAST -> HEAP -> FAST on one multi index: HEAP answers as a single HEAP index does, rows appended while
    HEAP is in force are in the FAST code image that is rebuilt afterwards; exact_ties = 1 changes nothing
    while FAST is in force"""
    c = make_case(7900, 64, [4] * 16, 30_000, 14, dup_frac=0.05)
    extra = make_case(7901, 64, [4] * 16, 3000, 1)["codes"]
    off, sc = quant_for(c)
    k = 50
    m = multi(c, 3, off, sc)
    v = fast_index(c, off, sc)
    lut = v.build_lut(c["X"])
    el, ed = fr.search_fast(lut, off, sc, c["codes"], k)
    same(m.search(c["X"], k), el, ed, "FAST")
    m.set_option("exact_ties", 1)
    same(m.search(c["X"], k), el, ed, "FAST, exact_ties = 1")
    m.set_option("exact_ties", 0)
    h = fast_index(c, off, sc, methods="HEAP")
    m.set_method(HEAP)
    a, b = m.search(c["X"], k), h.search(c["X"], k)
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.distances.view(np.uint32), b.distances.view(np.uint32))
    m.add_codes(extra)
    h.add_codes(extra)
    a, b = m.search(c["X"], k), h.search(c["X"], k)
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.distances.view(np.uint32), b.distances.view(np.uint32))
    m.set_method(FAST)
    c2 = dict(c, codes=np.concatenate([c["codes"], extra]))
    el, ed = fr.search_fast(lut, off, sc, c2["codes"], k)
    same(m.search(c["X"], k), el, ed, "FAST again, image rebuilt with the appended rows")
    v.add_codes(extra)
    same(v.search(c["X"], k), el, ed, "single")
    for x in (m, v, h):
        x.close()


def test_learn_quantization_on_the_multi_index(vaqlib):
    """learnt once on shard 0 and replicated: the same mOffsets / mScale bits as VaqHipFast.learnQuantization and
    as the checker's alpha loop (which tests/golden/fast/quantize.npz pins to the reference's); the golden
    quantisation itself, set by hand, searches alike on both"""
    from vaq_amd.index import VaqHipMulti
    c = make_case(8000, 64, [4] * 16, 30_000, 20)
    train = (np.random.default_rng(3).normal(size=(20000, 64)) * 30).astype(np.float32)
    v = fast_index(c)
    v.learnQuantization(train, 0.05)
    import vaq_amd
    m = VaqHipMulti([0, 0, 0], c["bits"], c["cents"], c["eig"])
    with pytest.raises(vaq_amd.VaqHipError) as e:
        m.set_method(FAST)  # no quantisation on the shards yet
    assert e.value.code == -2
    m.set_codes(c["codes"])
    off, sc = m.learn_quantization(train, 0.05)
    m.set_method(FAST)
    assert np.array_equal(off.view(np.uint32), v.mOffsets.view(np.uint32))
    assert np.array_equal(sc.view(np.uint32), v.mScale.view(np.uint32))
    eo, es, _ = fr.learn_from_luts(fr.stack_luts(v.build_lut(train[fr.sample_rows(train.shape[0], 0.05)])))
    assert np.array_equal(off, eo) and np.array_equal(sc, es)
    lut = v.build_lut(c["X"])
    el, ed = fr.search_fast(lut, off, sc, c["codes"], 100)
    same(m.search(c["X"], 100), el, ed, "learnt on the multi index")
    same(v.search(c["X"], 100), el, ed, "single")
    m.close()
    v.close()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast", "quantize.npz"))
    c8 = make_case(8001, 32, [4] * 8, 10_000, 9)
    check_all(c8, (2,), (100,), g["offsets"].astype(np.float32), g["scale"].astype(np.float32), what="golden quantisation")


@pytest.mark.parametrize("N,G,k,nq", [(500, 4, 17, 9), (3000, 3, 100, 5), (40, 2, 64, 3), (40_000, 16, 1024, 2), (7, 5, 1, 4)])
def test_merge_fast_device_on_hand_built_lists(vaqlib, N, G, k, nq):
    """vaqhip_merge_fast_device alone: the shards' parts built in NumPy (fast_multi_ref.shard_parts), merged on the
    GPU, against KNNFromDists over the whole array"""
    import torch
    from vaq_amd.index import merge_fast_device
    rng = np.random.default_rng(N + k)
    base = 777
    kk = min(k, N)
    bounds = fm.shard_bounds(N, G)
    head = np.zeros((nq, kk), np.uint16)
    ll = np.full((G, nq, k), -1, np.int32)
    ld = np.full((G, nq, k), fm.FLT_MAX, np.float32)
    el = np.empty((nq, k), np.int64)
    ed = np.empty((nq, k), np.float32)
    for q in range(nq):
        d = rng.integers(0, (2, 8, 4096)[q % 3], size=N).astype(np.int64) * 7
        for g, (lo, hi) in enumerate(bounds):
            pos, hd, rows, dd = fm.shard_parts(d, lo, hi, k)
            head[q, pos] = hd
            ll[g, q, :rows.shape[0]] = rows + base
            ld[g, q, :rows.shape[0]] = dd
        l, ed[q] = fr.knn_from_dists(d, k)
        el[q] = np.where(l >= 0, l + base, -1)
    lab, dis = merge_fast_device(torch.from_numpy(head.view(np.int16)).cuda(), torch.from_numpy(ld).cuda(),
                                 torch.from_numpy(ll).cuda(), k, head_label_base=base)
    torch.cuda.synchronize()
    assert np.array_equal(dis.cpu().numpy(), ed) and np.array_equal(lab.cpu().numpy(), el.astype(np.int32))


def test_cpp_adapter_with_devices_and_fast(vaqlib, tmp_path):
    """examples/demo_vaqhip.cpp with a FAST method string returns with --devices 0,0 (setDevices ->
    vaqhip_multi_*) what it returns without"""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    c = make_case(8100, 64, [4] * 16, 20_000, 15, dup_frac=0.05)
    dataset = (np.random.default_rng(4).normal(size=(8000, 64)) * 30).astype(np.float32)
    io.save_centroids(c["cents"], str(tmp_path / "c.bin"))
    io.save_codebook(c["codes"], str(tmp_path / "cb.bin"))
    c["eig"].astype(np.float32).tofile(str(tmp_path / "e.f32"))
    io.write_vecs(str(tmp_path / "q.fvecs"), c["X"])
    io.write_vecs(str(tmp_path / "base.fvecs"), dataset)
    got = {}
    for name, devs in (("single", []), ("two", ["--devices", "0,0"]), ("three", ["--devices", "0,0,0"])):
        out = str(tmp_path / f"{name}.csv")
        r = subprocess.run([exe, "--centroids", str(tmp_path / "c.bin"), "--codebook", str(tmp_path / "cb.bin"),
                            "--eigen", str(tmp_path / "e.f32"), "--queries", str(tmp_path / "q.fvecs"),
                            "--timeseries-size", "64", "--k", "100", "--method", "VAQ64m16min4max4var1,FAST",
                            "--dataset", str(tmp_path / "base.fvecs"), "--learn-ratio", "0.1", "--result", out] + devs,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got[name] = np.loadtxt(out, delimiter=",", dtype=np.int64)
    assert np.array_equal(got["two"], got["single"]) and np.array_equal(got["three"], got["single"])
    v = fast_index(c)
    v.learnQuantization(dataset, 0.1)
    assert np.array_equal(got["single"], v.search(c["X"], 100).labels.reshape(15, 100).astype(np.int64))
    v.close()
