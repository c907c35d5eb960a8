"""Option "exact_ties" on sequential-sum indexes (VaqHip(sequential_sum=True), the reference's
BitVecEngine::queryLUT): labels and distances identical to queryLUT's slot for slot, also where rows tie --
its choice among equal distances comes from libstdc++'s heap functions over k + 1 pairs
(BitVecEngine.hpp:1282-1317), replayed on the GPU (vaq_amd/csrc/vaq_exact.hip, vaq_restated.h stdheap).

Checked with plain array_equal on labels and bit equality on distances against the fixtures under
tests/golden/seq_exact/ (recorded from the loop over the real std::push_heap / pop_heap / sort_heap) and
against seq_exact_ref's restatement (pinned against both in tests/test_seq_exact_cpu.py, which also asserts
that the tie-heavy fixtures differ from the smallest-label rule: they fail without the replay)."""
import functools

import numpy as np
import pytest

import seq_exact_ref as sr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def inputs(name):
    return sr.make_inputs(name)


@functools.lru_cache(maxsize=None)
def all_dists(name):
    bits, cent, codes, X = inputs(name)
    return np.stack([sr.row_dists(X[q], bits, cent, codes) for q in range(sr.N_QUERIES)])


def make_index(name, n, exact=1, id_base=0):
    import vaq_amd
    bits, cent, codes, _ = inputs(name)
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = sr.centroid_list(bits, cent)
    v.id_base = id_base
    v.mCodebook = codes[:n]
    v.set_option("exact_ties", exact)
    return v


def same(a, k, want_l, want_d, what):
    nq = want_l.shape[0]
    lab, dis = a.labels.reshape(nq, k), a.distances.reshape(nq, k)
    assert np.array_equal(dis.view(np.uint32), want_d.view(np.uint32)), f"{what}: distances differ"
    bad = np.nonzero((lab != want_l).any(axis=1))[0]
    assert bad.size == 0, f"{what}: labels differ for queries {bad[:8]}: {lab[bad[0]]} vs {want_l[bad[0]]}"


def ref_topk(name, n, k, id_base=0):
    d = all_dists(name)
    out = [sr.query_lut_topk(d[q, :n], k) for q in range(sr.N_QUERIES)]
    lab = np.stack([o[0] for o in out])
    return np.where(lab >= 0, lab + id_base, -1).astype(np.int32), np.stack([o[1] for o in out])


@pytest.mark.parametrize("k", sr.KS)
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_fixtures_exactly(vaqlib, name, k):
    """N in {k - 1, k, k + 1, 300, 3000} (k = 1: an index without rows too), 33 queries and 1 query."""
    z = sr.load_fixture(name)
    X = inputs(name)[3]
    for n in sr.row_counts(k):
        want_l, want_d = z[f"labels_n{n}_k{k}"], z[f"dists_n{n}_k{k}"]
        v = make_index(name, n)
        same(v.search(X, k), k, want_l, want_d, f"{name} N={n} k={k}")
        for q in (0, 17):
            same(v.search(X[q:q + 1], k), k, want_l[q:q + 1], want_d[q:q + 1], f"{name} N={n} k={k}, query {q} alone")
        v.close()


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_projected_and_device_entries_and_scan_forms(vaqlib, name):
    """vaqhip_search_projected and vaqhip_search_device take the same path; the scan behind the option may be
    any form."""
    import torch
    k, n = 7, 3000
    z = sr.load_fixture(name)
    want_l, want_d = z[f"labels_n{n}_k{k}"], z[f"dists_n{n}_k{k}"]
    X = inputs(name)[3]
    v = make_index(name, n)

    class Pair:
        def __init__(self, labels, distances):
            self.labels, self.distances = labels, distances

    same(v.search(X, k, projected=True), k, want_l, want_d, f"{name} projected")
    l, d = v.search_device(torch.from_numpy(X).cuda(), k)
    torch.cuda.synchronize()
    same(Pair(l.cpu().numpy(), d.cpu().numpy()), k, want_l, want_d, f"{name} search_device")
    for qb, ea, bf in [(1, 1, 0), (2, 2, 1), (4, 0, 1)]:
        v.set_option("queries_per_pass", qb)
        v.set_option("early_abandon", ea)
        v.set_option("best_first", bf)
        same(v.search(X, k), k, want_l, want_d, f"{name} qb={qb} ea={ea} bf={bf}")
    v.close()


@pytest.mark.parametrize("name", sr.TIE_HEAVY)
def test_id_base_and_appended_rows(vaqlib, name):
    """The C ABI returns id_base + i; `i >= k` is about the row's position, not its label.  Rows appended
    later are replayed in their place."""
    k, base = 100, 70000
    X = inputs(name)[3]
    codes = inputs(name)[2]
    for n in (101, 300):
        v = make_index(name, n, id_base=base)
        same(v.search(X, k), k, *ref_topk(name, n, k, base), f"{name} id_base N={n}")
        v.close()
    v = make_index(name, 60, id_base=base)
    same(v.search(X, k), k, *ref_topk(name, 60, k, base), f"{name} before the append")
    v.add_codes(codes[60:101])   # the first k rows span both parts
    same(v.search(X, k), k, *ref_topk(name, 101, k, base), f"{name} after the first append")
    v.add_codes(codes[101:3000])
    same(v.search(X, k), k, *ref_topk(name, 3000, k, base), f"{name} after the second append")
    same(v.search(X, 7), 7, *ref_topk(name, 3000, 7, base), f"{name} after the second append, k=7")
    v.close()


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_option_off_is_the_unchanged_result(vaqlib, name):
    """Off (the default, and off again after on): the smallest-label order, bit for bit what an index that
    never saw the option returns."""
    k, n = 7, 3000
    X = inputs(name)[3]
    d = all_dists(name)
    plain = [sr.smallest_label_topk(d[q, :n], k) for q in range(sr.N_QUERIES)]
    want_l, want_d = np.stack([p[0] for p in plain]), np.stack([p[1] for p in plain])
    never = make_index(name, n, exact=0)
    same(never.search(X, k), k, want_l, want_d, f"{name} never on")
    v = make_index(name, n)
    z = sr.load_fixture(name)
    same(v.search(X, k), k, z[f"labels_n{n}_k{k}"], z[f"dists_n{n}_k{k}"], f"{name} on")
    v.set_option("exact_ties", 0)
    same(v.search(X, k), k, want_l, want_d, f"{name} off again")
    never.close()
    v.close()
