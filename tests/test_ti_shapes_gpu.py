"""ti_assign_kernel .. ti_bounds_kernel (the regroup of VAQ::clusterTI) and ti_plan_kernel (the per-query
cluster order) of vaq_amd/csrc/vaq_ti.hip at the shapes the scan tests do not bring with them:

  * every branch of l2sqr_ref_order -- d = 1, 2, 4, 8, 12 and the sequential loop at d = 3 and 16 -- on
    twin-centre inputs where the summation order decides which cluster a row joins and which twin a query
    visits first, through both addressing forms (rows in LDS, centres dimension-major);
  * every tier of ti_assign_lds at its edges: 256 / 128 / 64 rows per workgroup, 48 KB, just above, the
    128 KB LDS maximum, the global scratch tile, its grid-stride loop's second trip, N below one workgroup;
  * T = 1, 2, 3 (Tp = 2, 4), T on both sides of one pass of the bitonic network (511, 512, 513), 2000 and the
    limit 4096, with the visiting list staged in one chunk of up to 4096 entries; ti_plan_kernel<true>
    (option "exact_ties") at T = 600 and 4096.

Reference: the CPU oracle (oracle/vaq_oracle.c: vo_cluster_ti, vo_ti_query_order, vo_search_ti).
Bar: no tolerance anywhere.  Without EA (the answer is the first k rows of the visiting order) label sets
equal and distances bit-equal; with EA distances bit-equal and labels under the tie contract of
helpers.assert_topk_matches.  tests/test_ti_shapes_cpu.py shows that the twin cases have teeth and that
every tier case sits in its tier."""
import numpy as np
import pytest

from helpers import assert_topk_matches
from test_ti import _gpu_index, visited_dists

import ti_shapes_ref as ts

pytestmark = pytest.mark.gpu


def _search(v, c, k, ea, visit):
    from vaq_amd.index import NNMethod
    nq = c["X"].shape[0]
    v.mMethods = NNMethod.TI | (NNMethod.EA if ea else 0)
    v.mVisit = visit
    ans = v.search(c["X"], k, projected=True)
    return ans.labels.reshape(nq, k), ans.distances.reshape(nq, k)


def check_first_k(v, oracle, c, ti, k, what):
    """NNMethod.TI without EA: exactly the oracle's rows (the first k of the visiting order), its distances
    bit for bit, -1 / FLT_MAX where fewer than k rows exist."""
    lab, dis = _search(v, c, k, False, 0.3)
    ol, od, _ = oracle.search_ti(c["X"], c["cents"], ti, k, visit=0.3, ea=False, projected=True)
    assert np.array_equal(np.sort(lab, axis=1), np.sort(ol, axis=1)), f"{what} k={k}: other rows"
    assert_topk_matches(lab, dis, ol, od, what=f"{what} TI k={k}")


def check_ea(v, oracle, c, ti, k, visit, what, ties):
    lab, dis = _search(v, c, k, True, visit)
    ol, od, _ = oracle.search_ti(c["X"], c["cents"], ti, k, visit=visit, projected=True)
    alld = visited_dists(c, ti, visit, k) if ties else None
    assert_topk_matches(lab, dis, ol, od, all_dists=alld, what=f"{what} TI|EA visit={visit} k={k}")


# ----------------------------------------------------------- 1. summation orders --
@pytest.mark.parametrize("d", sorted(ts.TWIN_CASES))
def test_twin_centres_follow_the_reference_order(vaqlib, oracle, d):
    """The twin pair of every anchor is at equal true distance; which twin gets the anchor's rows, and which
    a query on the anchor visits first, is the last ulp of the fp32 sum.  Without EA at k = 1 and around the
    size of the first cluster visited the answer shows both; TI|EA at one cluster visited shows the plan's."""
    c = ts.twin_case(d)
    ti = ts.oracle_grouping(c)
    _, order = ts.oracle_orders(c)
    v = _gpu_index(c)
    for k in ts.twin_ks(c, ti, order):
        check_first_k(v, oracle, c, ti, k, f"twin d={d}")
    for visit in (1.0, 1.5 / ts.TWIN_T):  # every cluster; int(64 * visit) = 1 cluster
        for k in (1, 10):
            check_ea(v, oracle, c, ti, k, visit, f"twin d={d}", ties=True)
    info = v.info()
    assert info["ti_clusters"] == ts.TWIN_T and info["layout"] == (0 if len(c["bits"]) == 8 else 1), info
    v.close()


# ----------------------------------------------------------- 2. assign tiers --
@pytest.mark.parametrize("name", sorted(ts.TIER_CASES))
def test_assign_tier_groups_like_the_oracle(vaqlib, oracle, name):
    """One case per edge of ti_assign_lds (the tier each lands in is asserted in test_ti_shapes_cpu.py).
    d520_second_trip is the one large case: 131 137 rows, 273 MB of scratch tile on the device, the oracle
    on 8 threads."""
    d, seg, L, N, T, _ = ts.TIER_CASES[name]
    c = ts.tier_case(name)
    ti = ts.oracle_grouping(c, nthreads=8 if N > 15000 else 1)
    v = _gpu_index(c)
    for k in ts.tier_ks(N):
        check_first_k(v, oracle, c, ti, k, name)
    if N < 5:  # N < k: the tail is -1
        lab, _ = _search(v, c, 5, False, 0.3)
        assert np.all(lab[:, N:] == -1) and np.all(lab[:, :N] >= 0)
    check_ea(v, oracle, c, ti, 10, 1.0, name, ties=False)
    info = v.info()
    assert (info["ti_clusters"], info["ti_segments"], info["N"]) == (T, seg, N), info
    v.close()


def test_assign_refuses_centres_of_1025_dims(vaqlib):
    from vaq_amd import _lib
    _, d, seg, L = ts.TIER_REFUSED
    c = ts.ti_case(4999, 4 * L, ts.TIER_BITS, 70, 2, 4, seg)
    v = _gpu_index(c)
    with pytest.raises(_lib.VaqHipError) as e:
        v.search(c["X"], 1, projected=True)
    assert e.value.code == -2 and f"TI centres of {d} dims" in str(e.value)  # VAQHIP_EUNSUPPORTED
    v.close()


# ----------------------------------------------------------- 3. plan and visiting list --
_PLAN = {}


def plan_reference(oracle, T):
    if T not in _PLAN:
        c = ts.plan_case(T)
        _PLAN[T] = (c, ts.oracle_grouping(c))
    return _PLAN[T]


@pytest.mark.parametrize("T", ts.PLAN_T)
def test_plan_orders_clusters_like_the_oracle(vaqlib, oracle, T):
    """Visit 1.0 (the whole list staged in one chunk: 4096 entries, 80 KB of LDS, at the limit), 0.3 and one
    cluster; TI|EA at k = 1 and 100 (k > N at T <= 3), without EA at k = 7."""
    c, ti = plan_reference(oracle, T)
    v = _gpu_index(c)
    for visit in ts.plan_visits(T):
        for k in (1, 100):
            check_ea(v, oracle, c, ti, k, visit, f"T={T}", ties=T >= 511)
    check_first_k(v, oracle, c, ti, 7, f"T={T}")
    assert v.info()["ti_clusters"] == T
    v.close()


@pytest.mark.parametrize("option,value", [("waves_per_workgroup", 16), ("slices", 3)])
def test_plan_longest_list_split_and_merged(vaqlib, oracle, option, value):
    """T = 4096 at visit 1.0 and k = 100 once more with 16 waves per workgroup and with every query's units
    split over three workgroups and merged.  The plan accepts both (list, tables, top-k buffers and sixteen
    waves' queues are 117 824 B of the 160 KB of LDS) and a split happens either way."""
    T, k = 4096, 100
    c, ti = plan_reference(oracle, T)
    v = _gpu_index(c)
    v.set_option(option, value)
    v.set_option("timing", 1)
    lab, dis = _search(v, c, k, True, 1.0)
    t = v.last_timing()
    print(f"T={T} visit=1.0 k={k} {option}={value}: slices={t['slices']} lds_bytes={t['lds_bytes']}")
    assert t["slices"] == value if option == "slices" else t["slices"] > 1
    assert 4096 * 20 < t["lds_bytes"] <= 160 * 1024
    ol, od, _ = oracle.search_ti(c["X"], c["cents"], ti, k, visit=1.0, projected=True)
    assert_topk_matches(lab, dis, ol, od, all_dists=visited_dists(c, ti, 1.0, k), what=f"T={T} {option}={value}")
    v.close()


def test_plan_refuses_4097_clusters(vaqlib):
    from vaq_amd import _lib
    c = ts.ti_case(5999, 32, ts.PLAN_BITS, 70, 2, ts.MAX_TI_CLUSTERS + 1, 4)
    v = _gpu_index(c)
    with pytest.raises(_lib.VaqHipError) as e:
        v.search(c["X"], 1, projected=True)
    assert e.value.code == -2 and "4097" in str(e.value)  # VAQHIP_EUNSUPPORTED
    v.close()


@pytest.mark.parametrize("T", (513, 4096))
def test_visiting_order_row_by_row(vaqlib, oracle, T):
    """Not only the top-k: without EA the row that enters the answer at k is the oracle's k-th row of the
    visiting order (ti_query_order, then each cluster's members farthest first), k = 1 .. 32, two queries."""
    c, ti = plan_reference(oracle, T)
    c = dict(c, X=np.ascontiguousarray(c["X"][:2]))
    _, order = ts.oracle_orders(c)
    want = [ts.visiting_rows(ti["member"], ti["start"], order[q], 32) for q in range(2)]
    v = _gpu_index(c)
    seen = [set(), set()]
    for k in range(1, 33):
        lab, _ = _search(v, c, k, False, 0.3)
        for q in range(2):
            now = set(lab[q].tolist())
            assert len(now) == k and now - seen[q] == {int(want[q][k - 1])}, (T, q, k, sorted(now - seen[q]))
            seen[q] = now
    v.close()


@pytest.mark.parametrize("T", ts.EXACT_T)
def test_exact_plan_equals_the_default_where_nothing_ties(vaqlib, oracle, T):
    """ti_plan_kernel<true> above one pass of the network, its no-redo path and its extra LDS: on data without
    equal qToCCDist, equal member distances or equal distances in a top-(k + 1) (asserted on the spot and in
    test_ti_shapes_cpu.py) the reference's own order IS the ascending order, so option "exact_ties" must
    return the default answer bit for bit, labels included -- and that is the oracle's."""
    from test_ti_shapes_cpu import EXACT_COMBOS
    c = ts.exact_case(T)
    ti = ts.oracle_grouping(c)
    ts.check_no_ties(c, ti, EXACT_COMBOS)
    v = _gpu_index(c)
    for k, visit, ea in EXACT_COMBOS:
        v.set_option("exact_ties", 0)
        lab0, dis0 = _search(v, c, k, ea, visit)
        v.set_option("exact_ties", 1)
        lab1, dis1 = _search(v, c, k, ea, visit)
        ol, od, _ = oracle.search_ti(c["X"], c["cents"], ti, k, visit=visit, ea=ea, projected=True)
        what = f"T={T} k={k} visit={visit} ea={ea}"
        assert np.array_equal(lab0, ol) and np.array_equal(dis0.view(np.uint32), od.view(np.uint32)), what
        assert np.array_equal(lab1, lab0) and np.array_equal(dis1.view(np.uint32), dis0.view(np.uint32)), what
    v.close()
