"""Option "exact_ties" on a multi-device index of sequential-sum shards (VaqHipMulti(sequential_sum=True)):
BitVecEngine::queryLUT's answer over ALL rows slot for slot, identical to the single index's.  Shard g's
replay starts from the raw heap (k + 1 pairs, its length, bsfK) shards 0..g-1 left, and `dataIndex >= k`
counts from the shard's first global row (vaq_amd/csrc/vaqhip_multi_search.cpp, vaq_exact.hip); logical shards on
device 0 exercise every step.  Plain array_equal against the fixtures under tests/golden/seq_exact/ and
seq_exact_ref (tests/test_seq_exact_cpu.py pins both, and asserts that the tie-heavy fixtures differ from
the (distance, label) order the shards' merge follows)."""
import functools

import numpy as np
import pytest

import seq_exact_ref as sr

pytestmark = pytest.mark.gpu

DEVICES = [[0, 0, 0], [0, 0]]


@functools.lru_cache(maxsize=None)
def inputs(name):
    return sr.make_inputs(name)


@functools.lru_cache(maxsize=None)
def all_dists(name):
    bits, cent, codes, X = inputs(name)
    return np.stack([sr.row_dists(X[q], bits, cent, codes) for q in range(sr.N_QUERIES)])


def ref_topk(name, n, k, id_base=0):
    d = all_dists(name)
    out = [sr.query_lut_topk(d[q, :n], k) for q in range(sr.N_QUERIES)]
    lab = np.stack([o[0] for o in out])
    return np.where(lab >= 0, lab + id_base, -1).astype(np.int32), np.stack([o[1] for o in out])


def make_multi(devices, name, n, id_base=0, exact=1, **opts):
    from vaq_amd.index import VaqHipMulti
    bits, cent, codes, _ = inputs(name)
    m = VaqHipMulti(devices, list(bits), sr.centroid_list(bits, cent), sequential_sum=True)
    for key, val in opts.items():
        m.set_option(key, val)
    m.set_codes(codes[:n], id_base)
    m.set_option("exact_ties", exact)
    return m


def make_single(name, n, id_base=0):
    import vaq_amd
    bits, cent, codes, _ = inputs(name)
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = sr.centroid_list(bits, cent)
    v.id_base = id_base
    v.mCodebook = codes[:n]
    v.set_option("exact_ties", 1)
    return v


class Pair:
    def __init__(self, labels, distances):
        self.labels, self.distances = labels, distances


def same(a, k, want_l, want_d, what):
    nq = want_l.shape[0]
    lab, dis = a.labels.reshape(nq, k), a.distances.reshape(nq, k)
    assert np.array_equal(dis.view(np.uint32), want_d.view(np.uint32)), f"{what}: distances differ"
    bad = np.nonzero((lab != want_l).any(axis=1))[0]
    assert bad.size == 0, f"{what}: labels differ for queries {bad[:8]}: {lab[bad[0]]} vs {want_l[bad[0]]}"


def search_both(m, X, k, want_l, want_d, what):
    """through the host entry and through the device entry"""
    import torch
    same(m.search(X, k), k, want_l, want_d, what + " search")
    l, d = m.search_device(torch.from_numpy(X).cuda(), k)
    torch.cuda.synchronize()
    same(Pair(l.cpu().numpy(), d.cpu().numpy()), k, want_l, want_d, what + " search_device")


@pytest.mark.parametrize("devices", DEVICES, ids=[str(len(d)) for d in DEVICES])
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_shards_equal_the_fixtures_and_the_single_index(vaqlib, name, devices):
    """N = 250 with k = 100 on three shards (84 + 84 + 82 rows), N = 150 on two (75 + 75): the first k rows,
    which enter unconditionally, span two shards.  The recorded shapes besides."""
    z = sr.load_fixture(name)
    X = inputs(name)[3]
    G = len(devices)
    assert (250 + G - 1) // G < 100 or (150 + G - 1) // G < 100
    for k, n in [(100, 250), (100, 150), (100, 3000), (100, 101), (7, 300), (7, 8), (1, 2), (1, 3000)]:
        if n in (250, 150):
            want_l, want_d = ref_topk(name, n, k)
        else:
            want_l, want_d = z[f"labels_n{n}_k{k}"], z[f"dists_n{n}_k{k}"]
        m = make_multi(devices, name, n)
        search_both(m, X, k, want_l, want_d, f"{name} {G} shards N={n} k={k}")
        same(m.search(X[5:6], k), k, want_l[5:6], want_d[5:6], f"{name} {G} shards N={n} k={k}, one query")
        m.close()
        v = make_single(name, n)
        a = v.search(X, k)
        same(a, k, want_l, want_d, f"{name} single N={n} k={k}")
        v.close()


@pytest.mark.parametrize("name", sr.TIE_HEAVY)
def test_empty_shard_grown_last_shard_and_id_base(vaqlib, name):
    """Two rows on three shards leave one empty (it hands the heap on unchanged); rows appended later pile
    onto the LAST shard, whose first global row stays where it was; labels carry id_base, positions do not."""
    X = inputs(name)[3]
    codes = inputs(name)[2]
    base = 4000
    for k in (1, 7):
        m = make_multi([0, 0, 0], name, 2, id_base=base)
        assert m.info()["shard_rows"] == [1, 1, 0]
        search_both(m, X, k, *ref_topk(name, 2, k, base), f"{name} 2 rows on 3 shards, k={k}")
        m.close()
    k = 100
    m = make_multi([0, 0, 0], name, 90, id_base=base)
    search_both(m, X, k, *ref_topk(name, 90, k, base), f"{name} before the append")
    m.add_codes(codes[90:300])  # rows 90..99 enter unconditionally on the grown shard, 100.. do not
    assert m.info()["shard_rows"] == [30, 30, 240]
    search_both(m, X, k, *ref_topk(name, 300, k, base), f"{name} after the append")
    m.add_codes(codes[300:3000])
    search_both(m, X, k, *ref_topk(name, 3000, k, base), f"{name} after the second append")
    search_both(m, X, 7, *ref_topk(name, 3000, 7, base), f"{name} after the second append, k=7")
    m.close()


def test_several_batches_and_option_off(vaqlib):
    """"exact_batch" small: the 33 tied queries are replayed in several batches of the list.  Off: the
    shards' (distance, label) merge, bit for bit."""
    name, k, n = "grid_d6", 7, 3000
    z = sr.load_fixture(name)
    X = inputs(name)[3]
    want_l, want_d = z[f"labels_n{n}_k{k}"], z[f"dists_n{n}_k{k}"]
    for batch in (1, 4, 32, 0):
        m = make_multi([0, 0, 0], name, n, exact_batch=batch)
        search_both(m, X, k, want_l, want_d, f"exact_batch={batch}")
        m.close()
    d = all_dists(name)
    plain = [sr.smallest_label_topk(d[q, :n], k) for q in range(sr.N_QUERIES)]
    plain_l, plain_d = np.stack([p[0] for p in plain]), np.stack([p[1] for p in plain])
    m = make_multi([0, 0], name, n, exact=0)
    for exact in (0, 1, 0):
        m.set_option("exact_ties", exact)
        if exact:
            search_both(m, X, k, want_l, want_d, "on")
        else:
            search_both(m, X, k, plain_l, plain_d, "off")
    m.close()
