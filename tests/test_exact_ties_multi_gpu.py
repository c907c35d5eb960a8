"""Option "exact_ties" on the multi-device index: labels and distances identical to VAQ::search's over
ALL rows, slot for slot, although the rows are cut into shards.  The reference's heap after the rows of
shards 0..g is shard g's replay started from the heap shards 0..g-1 left behind, so the shards replay as
a chain (vaq_amd/csrc/vaqhip_multi_search.cpp, vaq_exact.hip); logical shards on device 0 exercise every step
of it.  Checked with plain array_equal against oracle.search (pinned against the reference's heap in
tests/test_oracle_golden.py) and the golden label lists.

What the inputs must offer for the comparison to mean something is asserted on the inputs themselves:
  * the (distance, label)-sorted top k differs from the reference's labels for some query -- the rule
    the shards' merge follows cannot give the answer.  Not possible for k = 1 (the heap admits on a
    strictly smaller distance, so both rules keep the first row of minimal distance); asserted for
    every other case;
  * some query has equal distances at ranks k and k + 1 carried by rows of two DIFFERENT shards -- a tie
    no shard can see alone (planted where the drawn case has none).  Needs a rank k + 1, so it is
    asserted where N > k."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import make_case

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = sorted(json.load(open(os.path.join(GOLD, "manifest.json"))).keys())

CONFIGS = [
    # seed, D, bits, N, nq, k, make_case kwargs: the tie-heavy ones of test_exact_ties_gpu.py
    (301, 16, [3] * 4, 5000, 16, 100, {"integer": True}),
    (302, 64, [4] * 8, 30000, 12, 100, {"integer": True, "rotate": False}),
    (303, 128, [8] * 8, 40000, 9, 100, {"dup_frac": 0.3}),
    (305, 128, [12, 10, 9, 8, 8, 7, 6, 4], 20000, 6, 100, {"dup_frac": 0.2}),
    (306, 64, [4] * 8, 90, 5, 100, {"integer": True, "rotate": False}),       # N < k
    (307, 64, [4] * 8, 100, 5, 100, {"integer": True, "rotate": False}),      # N == k
    (308, 64, [4] * 8, 3000, 7, 1, {"integer": True, "rotate": False}),       # k = 1
    (309, 64, [4] * 8, 70000, 4, 1000, {"integer": True, "rotate": False}),   # k near the maximum
]
DEVICES = [[0, 0], [0, 0, 0], [0] * 8]


def same(a, k, o_lab, o_dis, what):
    nq = o_lab.shape[0]
    lab, dis = a.labels.reshape(nq, k), a.distances.reshape(nq, k)
    assert np.array_equal(dis.view(np.uint32), o_dis.view(np.uint32)), f"{what}: distances differ"
    bad = np.nonzero((lab != o_lab).any(axis=1))[0]
    assert bad.size == 0, f"{what}: labels differ for queries {bad[:8]}: {lab[bad[0]]} vs {o_lab[bad[0]]}"


class Pair:
    def __init__(self, labels, distances):
        self.labels, self.distances = labels, distances


def case(seed, D, bits, N, nq, **kw):
    c = make_case(seed, D, bits, N, nq, **kw)
    if c["eig"] is None:
        c["eig"] = np.eye(D, dtype=np.float32)  # (small integers stay integers: sums are exact, ties everywhere)
    return c


def make_multi(devices, c, codes=None, exact=1, **opts):
    from vaq_amd.index import VaqHipMulti
    m = VaqHipMulti(devices, c["bits"], c["cents"], c["eig"])
    for key, val in opts.items():
        m.set_option(key, val)
    m.set_codes(c["codes"] if codes is None else codes)
    m.set_option("exact_ties", exact)
    return m


def search_both(m, X, k, o_lab, o_dis, what):
    """through the host entry and through the device entry"""
    import torch
    same(m.search(X, k), k, o_lab, o_dis, what + " search")
    l, d = m.search_device(torch.from_numpy(X).cuda(), k)
    torch.cuda.synchronize()
    same(Pair(l.cpu().numpy(), d.cpu().numpy()), k, o_lab, o_dis, what + " search_device")


def dists_of(oracle, c, Xp, q):
    return oracle.all_dists(oracle.create_lut(Xp[q], c["cents"], max(c["bits"])), c["codes"])


def sorted_by_dist_label(d, k):
    """rows of the k + 1 smallest (distance, label) pairs (fewer when there are fewer rows); NaN last"""
    order = np.lexsort((np.arange(d.size), d))
    return order[: k + 1]


def cross_shard_boundary_tie(d, k, per):
    o = sorted_by_dist_label(d, k)
    return o.size > k and d[o[k - 1]] == d[o[k]] and o[k - 1] // per != o[k] // per


def plant_cross_shard_tie(oracle, c, Xp, k, G, skip):
    """Make some query's rows at ranks k and k + 1 (by distance, then label) carry the same distance and
    lie in different shards, by copying one code row over a far row of another shard."""
    N = c["codes"].shape[0]
    per = (N + G - 1) // G
    qs = [q for q in range(Xp.shape[0]) if q not in skip]
    if any(cross_shard_boundary_tie(dists_of(oracle, c, Xp, q), k, per) for q in qs):
        return
    for q in qs:
        d = dists_of(oracle, c, Xp, q)
        o = sorted_by_dist_label(d, k)
        src = o[k - 1]
        if d[o[k]] == d[src]:
            # the tie is there, but its rows at ranks k and k + 1 share a shard: the rows of that shard that
            # follow rank k in the run take the code of a far row of another shard, so that rank k + 1
            # falls to the run's first row beyond the boundary
            end = (src // per + 1) * per
            run = np.nonzero(d == d[src])[0]
            if not np.any(run >= end):
                continue
            far = end + int(np.argmax(d[end:]))
            if d[far] <= d[src]:
                continue
            keep = c["codes"].copy()
            c["codes"][run[(run > src) & (run < end)]] = c["codes"][far]
            if cross_shard_boundary_tie(dists_of(oracle, c, Xp, q), k, per):
                return
            c["codes"][:] = keep
            continue
        for g in range(G):
            lo, hi = min(N, g * per), min(N, (g + 1) * per)
            if g == src // per or hi <= lo:
                continue
            for dst in (lo + int(np.argmax(d[lo:hi])), hi - 1, lo):
                if d[dst] <= d[src]:
                    continue
                keep = c["codes"][dst].copy()
                c["codes"][dst] = c["codes"][src]
                if cross_shard_boundary_tie(dists_of(oracle, c, Xp, q), k, per):
                    return
                c["codes"][dst] = keep
    raise AssertionError("no cross-shard tie could be planted")


@pytest.mark.parametrize("devices", DEVICES, ids=[str(len(d)) for d in DEVICES])
@pytest.mark.parametrize("seed,D,bits,N,nq,k,kw", CONFIGS, ids=[f"s{c[0]}" for c in CONFIGS])
def test_multi_exact_ties_matches_oracle(vaqlib, oracle, seed, D, bits, N, nq, k, kw, devices):
    """Before the chain existed 21 of these 24 cases failed (all but k = 1, where the two rules agree):
    every shard replayed the heap over its own rows and the lists were merged by (distance, label)."""
    G = len(devices)
    c = case(seed, D, bits, N, nq, **kw)
    c["X"][1] = np.nan  # FLT_MAX > NaN is false for every row: all slots stay -1 / FLT_MAX
    Xp = oracle.project(c["X"], c["eig"])
    per = (N + G - 1) // G
    if N > k:
        plant_cross_shard_tie(oracle, c, Xp, k, G, skip={1})
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True, nthreads=8)
    assert np.all(o_lab[1] == -1) and np.all(o_dis[1] == np.finfo(np.float32).max)
    # conditions on the inputs (module docstring)
    differs = cross = 0
    for q in range(nq):
        if q == 1:
            continue
        d = dists_of(oracle, c, Xp, q)
        by_label = sorted_by_dist_label(d, k)[:k]
        differs += int(not np.array_equal(by_label, o_lab[q][: by_label.size]))
        cross += int(cross_shard_boundary_tie(d, k, per))
    if k > 1:
        assert differs >= 1, "the smallest-label rule gives the reference's answer for every query: nothing is tested"
    if N > k:
        assert cross >= 1, "no query ties at ranks k / k + 1 across a shard boundary"
    m = make_multi(devices, c)
    assert m.info()["shard_rows"] == [max(0, min(N, (g + 1) * per) - min(N, g * per)) for g in range(G)]
    search_both(m, c["X"], k, o_lab, o_dis, f"{G} shards")
    m.close()


def test_after_add_codes_and_with_empty_shards(vaqlib, oracle):
    """Appended rows pile onto the LAST shard: shards stay contiguous label ranges, the chain holds.
    Five rows on eight shards: empty shards pass the heap on unchanged."""
    k = 100
    c = case(302, 64, [4] * 8, 30000, 12, integer=True, rotate=False)
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=4, projected=True, nthreads=8)
    m = make_multi([0, 0, 0], c, codes=c["codes"][:18000])
    h_lab, h_dis = oracle.search(Xp, c["cents"], c["codes"][:18000], k, max_bits=4, projected=True, nthreads=8)
    search_both(m, c["X"], k, h_lab, h_dis, "before the append")
    m.add_codes(c["codes"][18000:])
    assert m.info()["shard_rows"] == [6000, 6000, 18000]
    search_both(m, c["X"], k, o_lab, o_dis, "after the append")
    m.close()
    c = case(312, 64, [4] * 8, 5, 6, integer=True, rotate=False)
    c["codes"][3] = c["codes"][0]
    c["codes"][4] = c["codes"][1]
    Xp = oracle.project(c["X"], c["eig"])
    for k in (1, 2, 3, 4, 5, 9):
        o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=4, projected=True, nthreads=1)
        m = make_multi([0] * 8, c)
        assert m.info()["shard_rows"] == [1, 1, 1, 1, 1, 0, 0, 0]
        search_both(m, c["X"], k, o_lab, o_dis, f"5 rows on 8 shards, k={k}")
        m.close()


def test_several_batches_and_several_sets_of_queries(vaqlib, oracle):
    """The tied queries are replayed in batches of the list ("exact_batch" entries each) and a call is
    served in internal sets of 16384 queries: cross both."""
    k = 10
    c = case(301, 16, [3] * 4, 5000, 16, integer=True)
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=3, projected=True, nthreads=8)
    for batch in (1, 3, 5, 16, 0):
        m = make_multi([0, 0, 0], c, exact_batch=batch)
        search_both(m, c["X"], k, o_lab, o_dis, f"exact_batch={batch}")
        m.close()
    # 16384 + 16384 + 232 queries on few rows
    nq = 33000
    c = case(313, 16, [3] * 4, 600, nq, integer=True)
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=3, projected=True, nthreads=8)
    tied = sum(int(np.any(np.diff(o_dis[q]) == 0)) for q in range(0, nq, 97))
    assert tied >= 100, "the case is meant to have equal distances nearly everywhere"
    m = make_multi([0, 0, 0], c, exact_batch=100)
    search_both(m, c["X"], k, o_lab, o_dis, "three sets of queries")
    m.close()


@pytest.mark.parametrize("name", CASES)
def test_golden_labels_exactly_over_three_shards(vaqlib, name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    bits = z["bits"].tolist()
    c = dict(bits=bits, cents=[z[f"cent{s}"] for s in range(len(bits))], eig=z["eig"], codes=z["codes"])
    m = make_multi([0, 0, 0], c)
    seen = 0
    for key in z.files:
        if not key.startswith("labels_k"):
            continue
        k = int(key[len("labels_k"):])
        if k >= 1024:
            continue
        for bf in (1, 0):
            m.set_option("best_first", bf)
            same(m.search(z["X"], k), k, z[key], z[f"dists_k{k}"], f"{name} k={k} bf={bf}")
            seen += 1
    assert seen >= 2
    m.close()


def test_option_off_again_and_repeated_searches(vaqlib, oracle):
    """Off: the single index's default result bit for bit (nothing is left behind in the shards).
    A second search gives the first one's answer (buffers and events are reusable)."""
    import vaq_amd
    k = 100
    c = case(303, 128, [8] * 8, 40000, 9, dup_frac=0.3)
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(c["bits"])
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    ref = v.search(c["X"], k)
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=8)
    m = make_multi([0, 0, 0, 0], c, exact=0)
    for exact in (0, 1, 1, 0, 1, 0):
        m.set_option("exact_ties", exact)
        if exact:
            search_both(m, c["X"], k, o_lab, o_dis, "on")
        else:
            a = m.search(c["X"], k)
            assert np.array_equal(a.labels, ref.labels)
            assert np.array_equal(a.distances.view(np.uint32), ref.distances.view(np.uint32))
    m.close()
    v.close()


def test_a_failing_shard_with_the_option_set(vaqlib, oracle):
    """One shard of four refuses the search (its method is set to TI without clusters): the call returns
    that shard's error, nothing of the exchange or the chain was enqueued for anybody, the index answers
    rightly once the shard is repaired, and close() returns."""
    from vaq_amd import _lib
    k = 10
    c = case(303, 128, [8] * 8, 40000, 9, dup_frac=0.3)
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=8)
    m = make_multi([0, 0, 0, 0], c)
    search_both(m, c["X"], k, o_lab, o_dis, "before")
    L = _lib.load()
    L.vaqhip_index_set_method.argtypes = [C.c_void_p, C.c_uint, C.c_float]
    L.vaqhip_multi_shard.restype = C.c_void_p
    bad = C.c_void_p(m.shard(2))
    assert L.vaqhip_index_set_method(bad, 0x04 | 0x02, 1.0) == 0   # TI | EA, but no clusters were set
    for _ in range(3):
        with pytest.raises(_lib.VaqHipError) as e:
            m.search(c["X"], k)
        assert "shard 2" in str(e.value)
    assert L.vaqhip_index_set_method(bad, 0x80, 1.0) == 0          # HEAP again
    search_both(m, c["X"], k, o_lab, o_dis, "after the repair")
    m.close()


def test_multi_exact_ties_at_c2_size(vaqlib, oracle):
    """SIFT-1M shape (1M x 8 B, k = 100) on four shards, duplicates planted at each of eight queries' k-th
    distance and inside their top k (anywhere in the database: most pairs straddle shards)."""
    k, nq, N = 100, 72, 1_000_000
    c = make_case(7321, 128, [8] * 8, N, nq)
    Xp = oracle.project(c["X"], c["eig"])
    rng = np.random.default_rng(1)
    for q in range(8):
        d = oracle.all_dists(oracle.create_lut(Xp[q], c["cents"], 8), c["codes"])
        order = np.argpartition(d, k)[: k + 1]
        kth = order[np.argsort(d[order])[k - 1]]
        inner = order[np.argsort(d[order])[k // 2]]
        for dst in rng.integers(0, N, size=4):
            c["codes"][dst] = c["codes"][kth]
        for dst in rng.integers(0, N, size=2):
            c["codes"][dst] = c["codes"][inner]
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True, nthreads=8)
    m = make_multi([0, 0, 0, 0], c)
    for bf in (1, 0):
        m.set_option("best_first", bf)
        search_both(m, c["X"], k, o_lab, o_dis, f"planted ties bf={bf}")
    m.close()
