"""The scan kernels at the row widths the other files leave out: bit-packed rows of 4..8 dwords
(W = ceil(sum(bits) / 32)) through every form -- plain, queued, in place, spilled tables, TI and
best-first -- and the packing, bucketed reorder and append that index by W.

Reference: the CPU oracle on the unpacked uint16 codes (it shares nothing with the packing).
Bar: lookup tables bit-exact, distances bit-exact, labels under the tie contract of
helpers.assert_topk_matches.  There is no tolerance in this file.

tests/test_scan_widths_cpu.py restates the packing these kernels assume for the same table."""
import numpy as np
import pytest

from helpers import assert_topk_matches, make_case
from test_ti import _gpu_index, ti_case, visited_dists

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024  # bytes of LDS a workgroup can have on gfx950

# name -> (bits, N, nq).  D = L * M with L = 4 (L = 2 for M = 128); M % 4 == 0 throughout, so the
# best-first form is eligible; none is all-8-bit with M in (8, 16, 32), so every one is bit-packed.
# The name's digit is the row width in dwords, checked below.
CASES = {
    # (the non-uniform rows avoid groups of four that add up to 32 bits, which would align every field)
    "w4_bf": ([10, 8, 7, 8] * 2 + [8, 8, 7, 8] * 2, 4097, 9),     # 128 bits: fills dword 3 exactly
    "w5_bytes20": ([8] * 20, 5003, 33),                           # 160 bits: fills dword 4 exactly
    "w5_straddle": ([7] * 20, 4099, 7),                           # 140 bits: a field straddles every dword boundary
    "w6_ragged": ([8] * 19 + [9], 6007, 5),                       # 161 bits: one bit in dword 5, no field starts there
    "w6_full": ([12, 9, 7, 5] * 3 + [10, 9, 7, 5] * 3, 9001, 6),  # 192 bits, non-uniform
    "w7_straddle": ([7] * 28, 12007, 11),                         # 196 bits
    "w7_full": ([10, 7, 8, 8] * 3 + [9, 7, 8, 8] + [8, 7, 8, 8] * 3, 4999, 17),  # 224 bits
    "w8_resident": ([8] * 31 + [1], 19999, 5),   # 249 bits, 7938 table floats: all resident, word 7 decoded
    "w8_straddle": ([7, 7, 7, 6] * 9, 7003, 6),  # 243 bits, M = 36: a field across every boundary up to 6 / 7
    "w8_m128": ([2] * 128, 8191, 8),             # 256 bits, M = 128: the descriptor arrays are full
    # tables that cannot all sit in LDS even for one query per pass, while table 0 (8192 floats = 32 KiB)
    # does: 5 * 8192 + 4096 + 10 * 256 = 47 616 floats, 4 * 1 * 47 616 = 190 464 B > 163 840 B; 157 bits
    "w5_tail": ([13] * 5 + [12] + [8] * 10, 6001, 5),
    # 5 * 8192 + 4096 + 14 * 256 = 48 640 floats, 4 * 1 * 48 640 = 194 560 B > 163 840 B; 189 bits
    "w6_tail": ([13] * 5 + [12] + [8] * 14, 5009, 5),
    # 5 * 8192 + 4096 + 14 * 128 + 8 * 64 = 47 360 floats, 4 * 1 * 47 360 = 189 440 B > 163 840 B; 223 bits
    "w7_tail": ([13] * 5 + [12] + [7] * 14 + [6] * 8, 4673, 6),
}
TAIL = ("w5_tail", "w6_tail", "w7_tail")
RESIDENT = tuple(n for n in CASES if n not in TAIL)


def width(bits):
    return -(-sum(bits) // 32)


def lut_floats(bits):
    return sum(1 << b for b in bits)


for _name, (_bits, _N, _nq) in CASES.items():
    assert width(_bits) == int(_name[1]), (_name, sum(_bits))
    assert len(_bits) % 4 == 0 and all(1 <= b <= 15 for b in _bits), _name
    assert not (all(b == 8 for b in _bits) and len(_bits) in (8, 16, 32)), _name  # bit-packed layout
    assert 4097 <= _N <= 20000 and _N % 64 != 0 and 5 <= _nq <= 33, _name
    assert (4 * lut_floats(_bits) > LDS_LIMIT) == (_name in TAIL), _name
    assert 4 * (1 << _bits[0]) * 2 < LDS_LIMIT, _name  # table 0 alone fits, for two queries too
assert {width(b) for b, _, _ in CASES.values()} == {4, 5, 6, 7, 8}
assert 129 <= sum(CASES["w5_tail"][0]) <= 160 and 193 <= sum(CASES["w7_tail"][0]) <= 224
assert sum(CASES["w6_ragged"][0]) == 161 and sum(CASES["w6_full"][0]) == 192 and sum(CASES["w7_full"][0]) == 224


def dims(bits):
    return (2 if len(bits) == 128 else 4) * len(bits)


def make_index(c, id_base=0):
    import vaq_amd
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(c["bits"])
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    v.id_base = id_base
    return v


def oracle_all_dists(oracle, c, Xp, codes=None):
    codes = c["codes"] if codes is None else codes
    return np.stack([oracle.all_dists(oracle.create_lut(Xp[q], c["cents"], max(c["bits"])), codes)
                     for q in range(Xp.shape[0])])


_REF = {}


def reference(oracle, name):
    """The case and what the oracle says of it, computed once and shared (never written to)."""
    if name not in _REF:
        bits, N, nq = CASES[name]
        c = make_case(3100 + sum(bits) + len(bits), dims(bits), bits, N, nq, dup_frac=0.03)
        Xp = oracle.project(c["X"], c["eig"])
        ad = oracle_all_dists(oracle, c, Xp)
        top = {k: oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True) for k in (37, 1)}
        _REF[name] = (c, Xp, ad, top)
    return _REF[name]


def check_info(v, bits):
    info = v.info()
    assert info["layout"] == 1 and info["code_bytes"] == 4 * width(bits), info  # LAYOUT_BITS, W dwords per row
    assert info["lut_floats"] == lut_floats(bits)


# (queries_per_pass, slices, early_abandon, hot_buckets, best_first)
SWEEP = [(1, 0, 1, 16, 1), (1, 0, 1, 16, 0), (2, 0, 1, 16, 1), (4, 0, 1, 32, 1), (2, 3, 1, 5, 1), (1, 3, 1, 16, 1),
         (1, 0, 0, 16, 1), (2, 3, 0, 0, 1), (4, 0, 0, 16, 1), (1, 0, 2, 16, 1), (2, 3, 2, 32, 1), (4, 0, 2, 0, 1),
         (1, 0, 1, 0, 1)]


@pytest.mark.parametrize("name", RESIDENT)
def test_width_matches_oracle(vaqlib, oracle, name):
    """Tables bit-exact, then every form of the scan against the oracle: 1 / 2 / 4 queries per pass, no early
    abandon / queue / in place, one slice and three, best-first on and off (k = 37; k = 1 as well on two cases).
    The best-first form must have served at least one run of each case, and none where it was switched off."""
    bits, N, nq = CASES[name]
    c, Xp, ad, top = reference(oracle, name)
    v = make_index(c)
    check_info(v, bits)
    lut = v.build_lut(c["X"])
    o_lut = np.stack([oracle.create_lut(Xp[q], c["cents"], max(bits)) for q in range(nq)])
    assert np.array_equal(lut.view(np.uint32), o_lut.view(np.uint32))
    for k in (37, 1) if name in ("w6_ragged", "w8_resident") else (37,):
        o_lab, o_dis = top[k]
        bf_ran = 0
        for qb, slices, ea, hot, bf in SWEEP:
            v.set_option("queries_per_pass", qb)
            v.set_option("slices", slices)
            v.set_option("early_abandon", ea)
            v.set_option("hot_buckets", hot)
            v.set_option("best_first", bf)
            v.set_option("timing", 1)
            ans = v.search(c["X"], k)
            t = v.last_timing()
            v.set_option("timing", 0)
            assert t["best_first"] in (0, bf), (qb, slices, ea, hot, bf)
            bf_ran += t["best_first"]
            assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), o_lab, o_dis, ad,
                                what=f"{name} k={k} qb={qb} slices={slices} ea={ea} hot={hot} bf={bf}")
        assert bf_ran >= 1, (name, k, bf_ran)
    v.close()


@pytest.mark.parametrize("name", TAIL)
def test_width_tail_tables(vaqlib, oracle, name):
    """Allocations whose tables do not fit LDS even for one query (the arithmetic is next to the case table):
    the tail tables are read from global memory, queued, in place and without early abandon.  Four queries
    per pass have no such kernel: the planner must serve them two at a time, with the same results."""
    bits, N, nq = CASES[name]
    c, Xp, ad, top = reference(oracle, name)
    v = make_index(c)
    check_info(v, bits)
    k = 37
    o_lab, o_dis = top[k]
    for qb in (1, 2, 4):
        for ea, slices in ((0, 0), (1, 0), (2, 0), (1, 3), (2, 3)):
            v.set_option("queries_per_pass", qb)
            v.set_option("early_abandon", ea)
            v.set_option("slices", slices)
            v.set_option("timing", 1)
            ans = v.search(c["X"], k)
            t = v.last_timing()
            v.set_option("timing", 0)
            ran_qb = t["queries_per_pass"]
            assert ran_qb == min(qb, 2), (qb, ea, t)
            assert t["early_abandon"] == ea and t["best_first"] == 0, (qb, ea, t)
            # spilled: the workgroup's LDS is smaller than the tables of its queries alone would be
            assert t["lds_bytes"] <= LDS_LIMIT < 4 * ran_qb * lut_floats(bits), (qb, ea, t)
            assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), o_lab, o_dis, ad,
                                what=f"{name} qb={qb} ea={ea} slices={slices}")
    v.close()


# Slice counts with which the best-first form must have served a bucket-key setting.  Keys that are whole first
# codes (7 and 9 bits, 512 buckets with two bits of the second code, or the 2-bit code continued to 16 buckets)
# take its kernels with the shared first term (UL0); 512 small buckets also let three slices per query take it.
BF_KEYS = {("w5_straddle", 9): {1, 3}, ("w7_full", 9): {1, 3}, ("w8_m128", 9): {1}, ("w8_m128", 12): {1},
           ("w4_bf", 10): {1, 3}, ("w6_ragged", 9): {1, 3}, ("w8_straddle", 9): {1, 3}}
KEY_CASES = [(n, b) for n in ("w5_straddle", "w7_full", "w8_m128") for b in (1, 9, 12)] + \
            [("w4_bf", 10), ("w6_ragged", 9), ("w8_straddle", 9)]  # ... and those forms at W = 4, 6 and 8


@pytest.mark.parametrize("name,bucket_bits", KEY_CASES, ids=[f"{n}-{b}" for n, b in KEY_CASES])
def test_width_bucket_keys(vaqlib, oracle, name, bucket_bits):
    """The bucketed row order at a forced key width (2 buckets; 9 and 12 bits, which use up the 7-, 9- and
    2-bit first codes and continue into the second).  The reorder moves whole W-dword rows; results do not
    depend on it."""
    bits, N, nq = CASES[name]
    c, Xp, ad, top = reference(oracle, name)
    v = make_index(c)
    v._ensure_index()
    v.set_option("bucket_bits", bucket_bits)
    k = 37
    o_lab, o_dis = top[k]
    bf_slices = set()
    for qb, slices, ea, hot in [(1, 0, 1, 16), (2, 3, 1, 32), (4, 1, 2, 0), (2, 0, 2, 16), (1, 2, 0, 16), (1, 3, 1, 16)]:
        v.set_option("queries_per_pass", qb)
        v.set_option("slices", slices)
        v.set_option("early_abandon", ea)
        v.set_option("hot_buckets", hot)
        v.set_option("timing", 1)
        ans = v.search(c["X"], k)
        t = v.last_timing()
        v.set_option("timing", 0)
        if t["best_first"]:
            bf_slices.add(t["slices"])
        assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), o_lab, o_dis, ad,
                            what=f"{name} bucket_bits={bucket_bits} qb={qb} slices={slices} ea={ea} hot={hot}")
    assert bf_slices >= BF_KEYS.get((name, bucket_bits), set()), bf_slices
    v.close()


TI_CASES = dict({"w3_bytes12": [8] * 12},
                **{n: CASES[n][0] for n in ("w4_bf", "w5_straddle", "w6_full", "w7_full", "w8_resident")})
assert width(TI_CASES["w3_bytes12"]) == 3


@pytest.mark.parametrize("name", list(TI_CASES))
def test_width_ti(vaqlib, oracle, name):
    """scan_bits_ti_kernel<W> at W = 3 .. 8 against the oracle's restatement of clusterTI +
    searchTriangleInequality, as tests/test_ti.py checks its configurations (W = 1 and 2 there)."""
    bits = TI_CASES[name]
    N, nq, T, seg = 6007, 9, 40, 4
    c = ti_case(3300 + sum(bits), 4 * len(bits), bits, N, nq, T, seg)
    ti = oracle.cluster_ti(c["codes"], c["cents"], c["clusters"], seg)
    for visit in (1.0, 0.25, 0.05):
        v = _gpu_index(c, visit=visit)
        for k in (1, 10, 100):
            ans = v.search(c["X"], k, projected=True)
            ol, od, _ = oracle.search_ti(c["X"], c["cents"], ti, k, visit=visit, projected=True)
            alld = visited_dists(c, ti, visit, k) if max(bits) <= 4 else None
            assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), ol, od, all_dists=alld,
                                what=f"TI|EA {name} visit={visit} k={k}")
        info = v.info()
        assert info["ti_clusters"] == T and info["code_bytes"] == 4 * width(bits), info
        v.close()


@pytest.mark.parametrize("name", ["w5_bytes20", "w7_straddle"])
def test_width_appends(vaqlib, oracle, name):
    """Rows appended in three pieces, one of them a single row, no cut at a multiple of 64: merged into the
    bucketed order (the old rows twice the new ones, then the other way round) and -- from an empty index,
    the last piece four times what was there -- unpacked and regrouped.  Each equals one index over all
    rows bit for bit, and the oracle."""
    bits = CASES[name][0]
    N, nq, k = 17001, 8, 37
    c = make_case(3500 + sum(bits), dims(bits), bits, N, nq, dup_frac=0.03)
    full = c["codes"]
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], full, k, max_bits=max(bits), projected=True)
    ad = oracle_all_dists(oracle, c, Xp)
    ref = make_index(c)
    whole = ref.search(c["X"], k)
    assert_topk_matches(whole.labels.reshape(nq, k), whole.distances.reshape(nq, k), o_lab, o_dis, ad, what="whole")
    ref.close()
    # (an append is merged while the total stays below four times the rows last regrouped, 4096 at least)
    for first, cuts in ((7001, (7002, N)), (4271, (4272, N)), (0, (1001, 1002, N))):
        assert all(x % 64 != 0 for x in (first,) + cuts if x)
        v = make_index(dict(c, codes=full[:first]))
        a = v.search(c["X"], k)
        assert np.all(a.labels == -1) or first > 0
        lo = first
        for hi in cuts:
            v.add_codes(full[lo:hi])
            lo = hi
        assert v.info()["N"] == N
        for slices, ea, bf in ((0, 1, 1), (3, 1, 0), (0, 2, 1), (3, 0, 1)):
            v.set_option("slices", slices)
            v.set_option("early_abandon", ea)
            v.set_option("best_first", bf)
            b = v.search(c["X"], k)
            what = f"{name} first={first} cuts={cuts} slices={slices} ea={ea} bf={bf}"
            assert np.array_equal(b.labels, whole.labels), what
            assert np.array_equal(b.distances.view(np.uint32), whole.distances.view(np.uint32)), what
        assert_topk_matches(b.labels.reshape(nq, k), b.distances.reshape(nq, k), o_lab, o_dis, ad, what="appended")
        v.close()


FORMS = [(1, 1, 1), (1, 1, 0), (2, 2, 1), (4, 0, 1), (1, 2, 1)]  # (queries_per_pass, early_abandon, best_first)


def set_form(v, form):
    for key, val in zip(("queries_per_pass", "early_abandon", "best_first"), form):
        v.set_option(key, val)


@pytest.mark.parametrize("name", ["w6_ragged"])
def test_width_degenerate(vaqlib, oracle, name):
    """Six-dword rows at the edges of the row count: fewer rows than k, one planar tile of 64 rows +/- 1,
    every row identical, a NaN query."""
    bits = CASES[name][0]
    k = 37
    for N in (20, 63, 64, 65):  # N < k: the tail is -1 / FLT_MAX
        c = make_case(3700 + N, dims(bits), bits, N, 5, dup_frac=0.05)
        Xp = oracle.project(c["X"], c["eig"])
        o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True)
        ad = oracle_all_dists(oracle, c, Xp)
        v = make_index(c)
        for form in FORMS:
            set_form(v, form)
            ans = v.search(c["X"], k)
            lab = ans.labels.reshape(5, k)
            assert_topk_matches(lab, ans.distances.reshape(5, k), o_lab, o_dis, ad, what=f"{name} N={N} {form}")
            assert np.all(lab[:, N:] == -1) and np.all(lab[:, :min(N, k)] >= 0)
        v.close()
    # every row identical: all distances equal, the k smallest labels come back
    c = make_case(3801, dims(bits), bits, 4097, 5)
    c["codes"][:] = c["codes"][11]
    Xp = oracle.project(c["X"], c["eig"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=max(bits), projected=True)
    v = make_index(c)
    for form in FORMS:
        set_form(v, form)
        ans = v.search(c["X"], k)
        assert np.array_equal(ans.labels.reshape(5, k), np.tile(np.arange(k, dtype=np.int32), (5, 1))), form
        assert np.array_equal(ans.distances.reshape(5, k).view(np.uint32), o_dis.view(np.uint32)), form
    v.close()
    # a NaN query: no row is ever admitted; the other queries are served as usual
    c, Xp, ad, top = reference(oracle, name)
    nq = c["X"].shape[0]
    Xn = c["X"].copy()
    Xn[1, 3] = np.nan
    o_lab, o_dis = top[k]
    on_lab, _ = oracle.search(Xn, c["cents"], c["codes"], k, eig=c["eig"])
    assert np.all(on_lab[1] == -1)
    v = make_index(c)
    good = [q for q in range(nq) if q != 1]
    for form in FORMS:
        set_form(v, form)
        ans = v.search(Xn, k)
        lab, dis = ans.labels.reshape(nq, k), ans.distances.reshape(nq, k)
        assert np.all(lab[1] == -1), form
        assert_topk_matches(lab[good], dis[good], o_lab[good], o_dis[good], ad[good], what=f"{name} NaN query {form}")
    v.close()
