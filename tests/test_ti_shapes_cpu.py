"""What tests/test_ti_shapes_gpu.py relies on, checked without a GPU: the twin-centre cases really make the
summation order of fvec_L2sqr_ny observable (a kernel with the wrong order would change answers), every
tier case sits in the tier of ti_assign_lds it is named for, and the data of the exact_ties comparison has
no ties.  The counts asserted here are conditions on the inputs, not measurements of the kernels."""
import numpy as np
import pytest

from oracle import pyoracle as po

import ti_shapes_ref as ts

TEETH_D = (3, 4, 8, 12, 16)  # d = 1 and d = 2 have one order only: branch coverage, no teeth


@pytest.mark.parametrize("d", sorted(ts.TWIN_CASES))
def test_twin_case_is_what_it_claims(oracle, d):
    """Grid values, exact twins, own pair nearest; the numpy statement of the reference's order equals the
    oracle's (bit for bit after the sqrt the oracle hands out) and, where the reference is compiled, its
    fvec_L2sqr_ny on the twin vectors themselves; the non-EA cut points are well defined."""
    c = ts.twin_case(d)
    seg, L, bits, _ = ts.TWIN_CASES[d]
    assert c["clusters"].shape == (ts.TWIN_T, d) and c["codes"].shape == (ts.TWIN_N, len(bits))
    for a in c["cents"] + [c["X"]]:
        assert np.array_equal(a * 16, np.round(a * 16)) and np.abs(a).max() <= 4
    assert np.array_equal(c["clusters"] * 2.0 ** 20, np.round(c["clusters"] * 2.0 ** 20))
    ts.check_twins_nearest(c)
    Xr = ts.decode_rows(c)
    for a, rows in enumerate(c["anchor_rows"]):
        assert np.all(Xr[rows] == c["anchors"][a]) and 16 <= len(rows) < 48
    qcc, order = ts.oracle_orders(c)
    m_qcc, m_order = ts.model_query_order(c, ts.l2_ref_order)
    assert np.array_equal(qcc.view(np.uint32), m_qcc.view(np.uint32)) and np.array_equal(order, m_order)
    ti = ts.oracle_grouping(c)
    m_assign, m_member, m_start, m_xcc = ts.model_grouping(c, ts.l2_ref_order)
    assert np.array_equal(ti["member"], m_member) and np.array_equal(ti["start"], m_start)
    assert np.array_equal(ti["code2cc"].view(np.uint32), m_xcc.view(np.uint32))
    if po.have_ref():
        for a in range(len(c["anchors"])):
            want = po.ref_l2sqr_ny(c["anchors"][a], c["clusters"])
            assert np.array_equal(ts.l2_ref_order(c["anchors"][a], c["clusters"]).view(np.uint32), want.view(np.uint32))
            assert np.array_equal(np.sqrt(want).view(np.uint32), qcc[a].view(np.uint32))
        some = np.concatenate([r[:2] for r in c["anchor_rows"]] + [np.arange(0, ts.TWIN_N, 97)])
        for r in some:
            want = np.sqrt(po.ref_l2sqr_ny(Xr[r], c["clusters"]))
            assert want.min() == ti["code2cc"][r] and int(np.argmin(want)) == ts.oracle_assign(ti)[r]
    ts.check_cut_points(ti, qcc, order, ts.twin_ks(c, ti, order))
    # TI|EA: the oracle's pruned walk returns the k-min of the rows it may visit (nothing lost to rounding)
    for visit in (1.0, 1.5 / ts.TWIN_T):
        alld = np.sort(ts.visited_dists(c, ti, visit, 10), axis=1)[:, :10]
        _, od, _ = oracle.search_ti(c["X"], c["cents"], ti, 10, visit=visit, projected=True)
        assert np.array_equal(od.view(np.uint32), alld.view(np.uint32)), visit


@pytest.mark.parametrize("d", TEETH_D)
def test_twin_cases_have_teeth(oracle, d):
    """A kernel summing in the other order -- sequentially where the reference uses four lanes (d = 4, 8, 12),
    pairwise where it sums sequentially (d = 3, 16) -- would assign at least 4 anchors to the other twin, rank
    the twins of at least 4 queries the other way, and return other rows for at least 4 queries."""
    c = ts.twin_case(d)
    anchors, queries, answers = ts.twin_teeth(c)
    print(f"d={d}: the wrong order moves {anchors} of {ts.TWIN_ROW_ANCHORS} anchors, reorders the twins of "
          f"{queries} of {ts.TWIN_NQ} queries, changes the non-EA answer of {answers} queries")
    assert anchors >= 4 and queries >= 4 and answers >= 4


@pytest.mark.parametrize("d", (1, 2))
def test_one_order_only(d):
    """d = 1 and d = 2: every order gives the same sum (coverage of the two branches is all these cases add)."""
    assert ts.wrong_order(d) is None
    c = ts.twin_case(d)
    for a in c["anchors"]:
        assert np.array_equal(ts.l2_ref_order(a, c["clusters"]), ts.l2_sequential(a, c["clusters"]))


@pytest.mark.parametrize("name", sorted(ts.TIER_CASES))
def test_tier_cases_sit_in_their_tiers(name):
    d, seg, L, N, T, (rows, lds, trips) = ts.TIER_CASES[name]
    assert seg * L == d <= ts.MAX_TI_DIMS and seg <= len(ts.TIER_BITS) and 4 <= T <= 8
    got = ts.assign_tier(d) + (ts.tier_trips(d, N),)
    print(f"{name}: d={d} N={N} -> {got[0]} rows per workgroup, "
          f"{'global scratch' if got[1] == 0 else str(got[1]) + ' B of LDS'}, {got[2]} trip(s)")
    assert got == (rows, lds, trips), f"{name} no longer covers its tier: {got}"
    assert N <= 15000 or name == "d520_second_trip"


def test_tier_edges_are_edges():
    """Each edge of ti_assign_lds has a case on either side of it."""
    tiers = {d: ts.assign_tier(d) for d in (48, 49, 96, 97, 192, 193, 512, 513, 1024)}
    assert tiers[48] == (256, ts.ASSIGN_LDS_SOFT) and tiers[49][0] == 128
    assert tiers[96] == (128, ts.ASSIGN_LDS_SOFT) and tiers[97][0] == 64
    assert tiers[192] == (64, ts.ASSIGN_LDS_SOFT) and ts.ASSIGN_LDS_SOFT < tiers[193][1] <= ts.ASSIGN_LDS_MAX
    assert tiers[512] == (64, ts.ASSIGN_LDS_MAX) and tiers[513] == (64, 0) and tiers[1024] == (64, 0)
    assert {c[0] for c in ts.TIER_CASES.values()} >= set(tiers)
    assert ts.TIER_REFUSED[1] == ts.MAX_TI_DIMS + 1
    d, _, _, N, _, _ = ts.TIER_CASES["d520_second_trip"]
    assert -(-N // 64) == ts.ASSIGN_SCRATCH_GRID + 2 and N % 64 == 1  # two workgroups go round again, one for one row
    assert 2048 * 64 * d * 4 < 300e6  # the scratch tile of that case


def test_plan_cases_cover_the_network():
    """T on both sides of one pass of the bitonic network (Tp / 2 pairs on 256 threads), the smallest Tp,
    the limit; every visit of a case visits at least one cluster."""
    tp = {T: ts.plan_tp(T) for T in ts.PLAN_T}
    assert tp[1] == tp[2] == 2 and tp[3] == 4 and tp[511] == tp[512] == 512 and tp[513] == 1024 and tp[4096] == 4096
    assert tp[512] // 2 == ts.PLAN_THREADS < tp[513] // 2 and max(ts.PLAN_T) == ts.MAX_TI_CLUSTERS
    for T in ts.PLAN_T:
        assert ts.plan_rows(T) <= 12000
        v = min(ts.plan_visits(T))  # (0.3 of T <= 3 is no cluster at all: the until-k-rows rule alone)
        assert T <= 3 or (int(np.float32(T) * np.float32(v)) == 1 and v == ts.plan_visits(T)[-1])


EXACT_COMBOS = [(100, 1.0, True), (1, 0.3, True), (7, 0.3, False), (10, 0.05, True)]


@pytest.mark.parametrize("T", ts.EXACT_T)
def test_exact_cases_have_no_ties(oracle, T):
    """The data on which test_ti_shapes_gpu.py compares option "exact_ties" with the default label for label."""
    c = ts.exact_case(T)
    assert len(np.unique(c["clusters"], axis=0)) == T
    ts.check_no_ties(c, ts.oracle_grouping(c), EXACT_COMBOS)
