"""The multi-device refiner on the GPU (vaqhip_multi_refiner_*, vaqhip_multi_search_refine; the two kernels of
vaq_amd/csrc/vaq_refine.hip behind vaqhip_multi_refiner.cpp): the single refiner's answer slot for slot although the
raw rows are cut into shards.  Logical shards on device 0 exercise every step (broadcast, distances, gather, select).
Checked against the fixtures recorded from the reference's VAQ::refine (tests/golden/refine/), against
tests/refine_ref.py (pinned to those fixtures by test_refine_exact_cpu.py) and against the single refiner.

What the inputs must offer is asserted on the inputs themselves: on int_ties and r2048 the run of candidates whose
distance equals the k-th spans rows of at least two shards -- the case a per-shard selection followed by a merge would
get wrong, and a selection over the gathered distances in candidate order gets right."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import refine_ref as rr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEVICES = [[0, 0], [0, 0, 0], [0] * 8]
IDS = ["g2", "g3", "g8"]


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def run(refiner, Xq, cand, k, exact):
    refiner.exact_ties = exact
    ans = refiner.refine(Xq, cand, k)
    return ans.labels.reshape(len(Xq), k), ans.distances.reshape(len(Xq), k)


def check_both_rules(refiner, Xq, Xt, cand, k, id_base=0, what=""):
    for exact in (True, False):
        lab, dis = run(refiner, Xq, cand, k, exact)
        want_l, want_d = rr.refine(Xq, Xt, cand, k, exact=exact, id_base=id_base)
        assert bits_equal(dis, want_d), (what, exact)
        assert np.array_equal(lab, want_l), (what, exact)


def cut(N, G):
    """shard of every row under the multi index's cut: rows [g * ceil(N / G), (g + 1) * ceil(N / G))"""
    per = max(-(-N // G), 1)
    return np.arange(N) // per


def cross_shard_ties(d, cand, k, G, N):
    """queries on which the candidates at the k-th smallest distance hold rows of at least two shards"""
    shard = cut(N, G)
    n = 0
    for q in range(len(cand)):
        kth = np.sort(d[q])[k - 1]
        n += len(set(shard[cand[q][d[q] == kth]])) >= 2
    return n


@functools.lru_cache(maxsize=None)
def case(name):
    Xq, Xt, cand = rr.make_inputs(name)
    return Xq, Xt, cand, rr.distances(Xq, Xt, cand)


def multi_refiner(devices, Xt, id_base=0):
    import vaq_amd
    r = vaq_amd.VaqMultiRefiner(devices, Xt.shape[1])
    r.set_rows(Xt, id_base=id_base)
    return r


@pytest.mark.parametrize("devices", DEVICES, ids=IDS)
@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_goldens(vaqlib, name, devices):
    """Every recorded answer on 2, 3 and 8 shards: with exact_ties labels and distances slot for slot; without, the
    default rule's relation to the fixture and equality with the restated (distance, label) rule."""
    c = rr.CASES[name]
    Xq, Xt, cand, d = case(name)
    G = len(devices)
    # every shard holds some of every query's candidates
    shard = cut(c["N"], G)
    if not c["dup"] and c["R"] >= 200:
        assert all(len(set(shard[row])) == G for row in cand)
    if name in ("int_ties", "r2048"):
        for k in (k for k in c["ks"] if k < c["R"] and k <= 100):
            assert cross_shard_ties(d, cand, k, G, c["N"]) == c["nq"], (name, k, G)
    r = multi_refiner(devices, Xt)
    assert sum(r.info()["shard_rows"]) == c["N"] and r.info()["n_devices"] == G
    z = rr.load_fixture(name)
    for k in c["ks"]:
        want_l, want_d = z[f"labels_k{k}"], z[f"dists_k{k}"]
        lab, dis = run(r, Xq, cand, k, True)
        assert bits_equal(dis, want_d), (name, k)
        assert np.array_equal(lab, want_l), (name, k)
        lab, dis = run(r, Xq, cand, k, False)
        rr.assert_default_rule(lab, dis, want_l, want_d, what=f"{name} k={k}")
        sl = np.stack([rr.smallest_label_topk(d[q], cand[q], k)[0] for q in range(len(cand))])
        assert np.array_equal(lab, sl), (name, k)
    r.close()


def test_inputs_have_cross_shard_ties():
    """the counts the comparison above rests on, for every one of the three cuts"""
    for G in (2, 3, 8):
        _, _, cand, d = case("int_ties")
        assert [cross_shard_ties(d, cand, k, G, 300) for k in (1, 10, 100)] == [6, 6, 6], G
        _, _, cand, d = case("r2048")
        assert [cross_shard_ties(d, cand, k, G, 3000) for k in (1, 100)] == [2, 2], G


@functools.lru_cache(maxsize=None)
def shape_rows():
    """the 500 x 20 rows of test_refine_exact_gpu.shape_rows: one packet and a tail of 4, 80-byte rows, built from 25
    distinct vectors with a little noise so that equal and nearly equal distances occur"""
    rng = np.random.default_rng(77)
    base = rng.integers(0, 64, size=(25, 20)).astype(np.float32)
    Xt = base[rng.integers(0, 25, 500)]
    Xt[::3] += rng.uniform(-1e-3, 1e-3, size=Xt[::3].shape).astype(np.float32)
    Xq = rng.integers(0, 64, size=(65, 20)).astype(np.float32)
    return Xq, np.ascontiguousarray(Xt)


@pytest.fixture(scope="module")
def shape_refiner(vaqlib):
    r = multi_refiner([0, 0, 0], shape_rows()[1])
    yield r
    r.close()


@pytest.mark.parametrize("R", [1, 3, 16, 17, 200, 2048])
@pytest.mark.parametrize("nq", [1, 3, 65])
def test_shapes(shape_refiner, nq, R):
    """one query and more than a wave's worth; R below, at and just past the 16 candidate groups of a workgroup, no
    power of two, and the limit; k = 1 and k = R; on 3 shards (167 + 167 + 166 rows)"""
    Xq, Xt = shape_rows()
    rng = np.random.default_rng(1000 * nq + R)
    cand = rng.integers(0, 500, size=(nq, R)).astype(np.int32)
    for k in sorted({1, R}):
        check_both_rules(shape_refiner, Xq[:nq], Xt, cand, k, what=(nq, R, k))


def test_cuts(vaqlib):
    """empty shards (N < G), rows that arrive by add_rows alone, candidates on the first and last row of every shard,
    id_base = 1000"""
    import vaq_amd
    Xq, Xt, _, _ = case("cont_d40")
    # N = 5 on 8 devices: shards 5..7 are empty
    r = multi_refiner([0] * 8, Xt[:5], id_base=1000)
    assert r.info()["shard_rows"] == [1, 1, 1, 1, 1, 0, 0, 0]
    cand = (1000 + np.array([[4, 0, 2, 3, 1, 4, 0]] * len(Xq))).astype(np.int32)
    check_both_rules(r, Xq, Xt[:5], cand, 3, id_base=1000, what="N=5 G=8")
    # N = 0, then add_rows: everything sits on the last shard
    r.set_rows(Xt[:0], id_base=1000)
    assert r.info()["N"] == 0 and r.info()["shard_rows"] == [0] * 8
    lab, dis = run(r, Xq, cand, 3, True)
    assert np.all(lab == -1) and np.all(dis == rr.FLT_MAX)
    r.add_rows(Xt[:40])
    assert r.info()["shard_rows"] == [0] * 7 + [40]
    cand = (1000 + np.stack([np.random.default_rng(q).permutation(40)[:24] for q in range(len(Xq))])).astype(np.int32)
    check_both_rules(r, Xq, Xt[:40], cand, 8, id_base=1000, what="N=0 + add_rows")
    r.close()
    # first and last row of every shard, for every cut
    for devices in DEVICES:
        G = len(devices)
        r = multi_refiner(devices, Xt, id_base=1000)
        rows = r.info()["shard_rows"]
        assert sum(rows) == 300 and min(rows) > 0
        ends = np.cumsum([0] + rows)
        edge = np.array(sorted({int(e) for e in ends[:-1]} | {int(e) - 1 for e in ends[1:]}))
        assert len(edge) == 2 * G
        cand = (1000 + np.stack([np.random.default_rng(q).permutation(edge) for q in range(len(Xq))])).astype(np.int32)
        for k in (1, G, 2 * G):
            check_both_rules(r, Xq, Xt, cand, k, id_base=1000, what=("edges", G, k))
        r.close()


def test_add_rows_grow_the_last_shard(vaqlib):
    """set_rows of 120 rows, then two add_rows: the last shard grows; candidates on both sides of the old end"""
    Xq, Xt, _, _ = case("cont_d129")
    for devices in DEVICES:
        G = len(devices)
        r = multi_refiner(devices, Xt[:120], id_base=1000)
        before = r.info()["shard_rows"]
        r.add_rows(Xt[120:250])
        r.add_rows(Xt[250:])
        after = r.info()["shard_rows"]
        assert after[:-1] == before[:-1] and after[-1] == before[-1] + 180 and r.info()["N"] == 300
        rng = np.random.default_rng(9)
        cand = (1000 + np.stack([rng.permutation(np.arange(100, 300))[:64] for _ in range(len(Xq))])).astype(np.int32)
        assert (cand >= 1250).any() and (cand < 1120).any()
        check_both_rules(r, Xq, Xt, cand, 16, id_base=1000, what=("appended", G))
        r.close()
    import vaq_amd
    r = vaq_amd.VaqMultiRefiner([0, 0], 129)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        r.set_rows(Xt, id_base=2**31 - 10)
    assert e.value.code == -6  # VAQHIP_ERANGE
    r.close()


@pytest.mark.parametrize("devices", DEVICES, ids=IDS)
def test_skipped_labels(vaqlib, devices):
    """the list of test_refine_exact_gpu.test_skipped_labels: negative labels, labels below id_base and past the end,
    in the host form and in the device form, whose select kernel finds no owner for them"""
    import torch
    Xq, Xt, cand, _ = case("cont_d40")
    k = 10
    r = multi_refiner(devices, Xt, id_base=1000)
    clean = cand + 1000
    mixed = np.insert(clean, [0, 5, 50, 200], [-7, 999, 1300, 2**31 - 1], axis=1).astype(np.int32)
    assert mixed.shape[1] == cand.shape[1] + 4
    for exact in (True, False):
        want_l, want_d = rr.refine(Xq, Xt, clean, k, exact=exact, id_base=1000)
        lab, dis = run(r, Xq, mixed, k, exact)
        assert np.array_equal(lab, want_l) and bits_equal(dis, want_d), exact
        dl, dd = r.refine_device(torch.from_numpy(Xq).cuda(), torch.from_numpy(mixed).cuda(), k)
        torch.cuda.synchronize()
        assert np.array_equal(dl.cpu().numpy(), want_l) and bits_equal(dd.cpu().numpy(), want_d), exact
        # nothing admissible at all: every slot unfilled
        lab, dis = run(r, Xq, np.array([[-1, 5, 1300]] * len(Xq), np.int32), 2, exact)
        assert np.all(lab == -1) and np.all(dis == rr.FLT_MAX)
    r.close()


@pytest.mark.parametrize("G", [1, 2, 8])
def test_equals_the_single_refiner(vaqlib, G):
    """the same inputs through VaqRefiner and through 1, 2 and 8 shards: labels and distance bits, both rules, host
    and device forms; with option "timing" the phases are reported and the answer is the same"""
    import torch
    import vaq_amd
    Xq, Xt, cand, _ = case("int_ties")
    one = vaq_amd.VaqRefiner(Xt.shape[1])
    one.set_rows(Xt)
    r = multi_refiner([0] * G, Xt)
    for exact in (True, False):
        for k in (1, 10, 200):
            want_l, want_d = run(one, Xq, cand, k, exact)
            lab, dis = run(r, Xq, cand, k, exact)
            assert np.array_equal(lab, want_l) and bits_equal(dis, want_d), (G, exact, k)
            dl, dd = r.refine_device(torch.from_numpy(Xq).cuda(), torch.from_numpy(cand).cuda(), k)
            torch.cuda.synchronize()
            assert np.array_equal(dl.cpu().numpy(), want_l) and bits_equal(dd.cpu().numpy(), want_d), (G, exact, k)
    assert r.info()["last_sets"] == 0
    r.set_option("timing", 1)
    lab, dis = run(r, Xq, cand, 10, True)
    inf = r.info()
    assert inf["last_sets"] == 1 and inf["last_distances_ms"] > 0 and (G == 1 or inf["last_select_ms"] > 0)
    want_l, want_d = run(one, Xq, cand, 10, True)
    assert np.array_equal(lab, want_l) and bits_equal(dis, want_d)
    r.close()
    one.close()


def test_more_than_one_set(vaqlib):
    """nq = 2 * 16384 + 5 on 3 shards: a _device call of three sets (the third of 5 queries), the host form in three
    staged calls; int_ties tiled, so every query still ties across the cuts (test_inputs_have_cross_shard_ties).  The
    expected answer is computed on the 6 distinct queries and tiled.  Under "timing" the three sets are reported, the
    answer is the same, and a small call afterwards reports one set again."""
    import torch
    import vaq_amd
    Xq, Xt, cand, _ = case("int_ties")
    r = multi_refiner([0, 0, 0], Xt)
    SET = r.info()["set_queries"]
    assert SET == 16384
    nq = 2 * SET + 5
    pick = np.arange(nq) % len(Xq)
    Xq_t, cand_t = np.ascontiguousarray(Xq[pick]), np.ascontiguousarray(cand[pick])
    dq, dc = torch.from_numpy(Xq_t).cuda(), torch.from_numpy(cand_t).cuda()
    one = vaq_amd.VaqRefiner(Xt.shape[1])
    one.set_rows(Xt)

    def device_form(k):
        dl, dd = r.refine_device(dq, dc, k)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dd.cpu().numpy()

    for exact in (True, False):
        for k in (1, 10):
            want_l, want_d = rr.refine(Xq, Xt, cand, k, exact=exact)
            want_l, want_d = want_l[pick], want_d[pick]
            lab, dis = run(r, Xq_t, cand_t, k, exact)
            assert np.array_equal(lab, want_l) and bits_equal(dis, want_d), (exact, k, "host form")
            lab, dis = device_form(k)
            assert np.array_equal(lab, want_l) and bits_equal(dis, want_d), (exact, k, "device form")
            lab, dis = run(one, Xq_t, cand_t, k, exact)
            assert np.array_equal(lab, want_l) and bits_equal(dis, want_d), (exact, k, "single refiner")
    assert r.info()["last_sets"] == 0
    r.set_option("timing", 1)
    lab, dis = device_form(10)  # (exact_ties is off since the loop's last round)
    inf = r.info()
    assert inf["last_sets"] == 3 and inf["last_distances_ms"] > 0 and inf["last_select_ms"] > 0, inf
    assert np.array_equal(lab, want_l) and bits_equal(dis, want_d)
    dl, dd = r.refine_device(dq[:3], dc[:3], 10)
    torch.cuda.synchronize()
    assert r.info()["last_sets"] == 1
    assert np.array_equal(dl.cpu().numpy(), want_l[:3]) and bits_equal(dd.cpu().numpy(), want_d[:3])
    r.close()
    one.close()


def golden_multi(name, exact, devices):
    from vaq_amd.index import VaqHipMulti
    z = np.load(os.path.join(GOLD, name + ".npz"))
    bits = [int(b) for b in z["bits"]]
    m = VaqHipMulti(devices, bits, [z[f"cent{s}"] for s in range(len(bits))], z["eig"])
    m.set_codes(z["codes"])
    m.set_option("exact_ties", 1 if exact else 0)
    return m, z


def fused_base(z):
    X = z["X"]
    N, D = z["codes"].shape[0], X.shape[1]
    base = (np.random.default_rng(5).uniform(-40, 40, size=(N, D))).astype(np.float32) + X[0]
    base[::7] = base[3]  # equal rows: equal refined distances
    return base


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", ["d128_m8_b8", "d128_m32_b78"])
def test_fused_search_refine(vaqlib, oracle, name, exact):
    """VaqHipMulti.search_refine(R = 100, k = 10) on 3 shards == search(100) + VaqMultiRefiner.refine == the
    restatement over the oracle's search result, with exact_ties on both objects and with it off; the same through
    the _device entry"""
    import torch
    devices = [0, 0, 0]
    m, z = golden_multi(name, exact, devices)
    X = z["X"]
    base = fused_base(z)
    r = multi_refiner(devices, base)
    r.exact_ties = exact
    fused = m.search_refine(X, 100, 10, r)
    cand = m.search(X, 100)
    two = r.refine(X, cand, 10)
    assert np.array_equal(fused.labels, two.labels) and bits_equal(fused.distances, two.distances)
    o_lab, _ = oracle.search(X, [z[f"cent{s}"] for s in range(len(z["bits"]))], z["codes"], 100, eig=z["eig"])
    if exact:
        assert np.array_equal(cand.labels.reshape(o_lab.shape), o_lab)
    want_l, want_d = rr.refine(X, base, o_lab, 10, exact=exact)
    assert np.array_equal(fused.labels.reshape(want_l.shape), want_l)
    assert bits_equal(fused.distances.reshape(want_d.shape), want_d)
    dl, dd = m.search_refine_device(torch.from_numpy(X).cuda(), 100, 10, r)
    torch.cuda.synchronize()
    assert np.array_equal(dl.cpu().numpy(), want_l) and bits_equal(dd.cpu().numpy(), want_d)
    r.close()
    m.close()


def test_refusals(vaqlib):
    import vaq_amd
    m, z = golden_multi("d128_m8_b8", False, [0, 0])
    X = z["X"]
    N, D = z["codes"].shape[0], X.shape[1]

    def refused(r, R=100, k=10):
        with pytest.raises(vaq_amd.VaqHipError) as e:
            m.search_refine(X, R, k, r)
        return e.value.code

    r = multi_refiner([0, 0], np.zeros((N - 1, D), np.float32))
    assert refused(r) == -7  # VAQHIP_ESTATE: N differs
    r.set_rows(np.zeros((N, D), np.float32), id_base=3)
    assert refused(r) == -7  # id_base differs
    r.set_rows(np.zeros((N, D), np.float32))
    assert refused(r, R=2048) == -2  # R > VAQHIP_MAX_K
    assert refused(r, R=2049) == -2 and refused(r, R=5, k=6) == -2 and refused(r, k=0) == -1
    m.search_refine(X, 100, 10, r)
    for other in (multi_refiner([0, 0, 0], np.zeros((N, D), np.float32)), multi_refiner([0], np.zeros((N, D), np.float32)),
                  multi_refiner([0, 0], np.zeros((N, D + 1), np.float32))):
        assert refused(other) == -1  # the device lists differ; D differs
        other.close()
    # the refiner's own limits, and nq = 0
    out_l, out_d = np.full(4, 77, np.int32), np.full(4, 7.0, np.float32)
    q = np.zeros((1, D), np.float32)
    lin = np.zeros(4096, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert vaqlib.vaqhip_multi_refiner_refine(r._h, p(q), 1, p(lin), 2049, 2, p(out_l), p(out_d)) == -2  # R > 2048
    assert vaqlib.vaqhip_multi_refiner_refine(r._h, p(q), 1, p(lin), 4, 5, p(out_l), p(out_d)) == -2  # k > R
    assert vaqlib.vaqhip_multi_refiner_refine(r._h, p(q), 1, p(lin), 4, 0, p(out_l), p(out_d)) == -1
    assert vaqlib.vaqhip_multi_refiner_refine(r._h, p(q), -1, p(lin), 4, 2, p(out_l), p(out_d)) == -1
    assert vaqlib.vaqhip_multi_refiner_refine(r._h, p(q), 0, p(lin), 4, 2, p(out_l), p(out_d)) == 0  # nq = 0
    assert vaqlib.vaqhip_multi_search_refine(m._h, r._h, p(q), 0, 4, 2, p(out_l), p(out_d)) == 0
    assert np.all(out_l == 77) and np.all(out_d == 7.0)
    ans = r.refine(np.empty((0, D), np.float32), np.empty(0, np.int32), 3)
    assert ans.labels.size == 0 and ans.distances.size == 0
    r.close()
    m.close()


def test_cpp_shim(vaqlib, tmp_path):
    """VaqHip::search(X, 10, 100) after setDevices({0, 0, 0}) and setRefineDataset equals the single-device shim's
    answer (tests/cpp/refine_multi_shim_test.cpp)."""
    from helpers import make_case
    from vaq_amd import build
    N, M, L, bits, nq = 6000, 8, 4, 8, 9
    c = make_case(733, M * L, [bits] * M, N, nq, dup_frac=0.2, rotate=False)
    rng = np.random.default_rng(3)
    base = rng.uniform(-30, 30, size=(N, M * L)).astype(np.float32)
    base[rng.integers(0, N, 2000)] = base[rng.integers(0, N, 2000)]
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([N, M, L, bits, nq], np.int32).tobytes())
        f.write(np.ascontiguousarray(c["codes"]).tobytes())
        for cent in c["cents"]:
            f.write(np.ascontiguousarray(cent, np.float32).tobytes())
        f.write(base.tobytes())
        f.write(np.ascontiguousarray(c["X"], np.float32).tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "refine_multi_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "refine_multi_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refine_multi_shim ok" in r.stdout, r.stdout + r.stderr


def test_cpp_demo_refine_resident_devices(vaqlib, oracle, tmp_path):
    """demo_vaqhip --devices 0,0 --refine 100,200 --refine-resident --exact-ties 1 on the data of
    test_cpp_demo_refine_resident: the label files the restatement predicts from the oracle's search result"""
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
                        "--method", "VAQ64m8min8max8var1,HEAP", "--devices", "0,0", "--refine", "100,200",
                        "--refine-resident", "--exact-ties", "1", "--dataset-refine", str(tmp_path / "base.fvecs"),
                        "--result", str(tmp_path / "out.csv")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "Refine = 200 (resident rows, fused with the search)" in r.stdout and "20000 rows resident" in r.stdout
    assert "shard 0 (device 0): 10000 rows resident" in r.stdout and "shard 1 (device 0): 10000 rows resident" in r.stdout
    for R in (100, 200):
        got = np.loadtxt(str(tmp_path / f"out.csv_R{R}"), delimiter=",", dtype=np.int64)
        cand, _ = oracle.search(c["X"], c["cents"], c["codes"], R)
        want_l, _ = rr.refine(c["X"], base, cand, 100)
        assert np.array_equal(got, want_l), R
