"""The numpy references of tests/primitives_ref.py against the compiled oracle, on a reduced grid of the
shapes tests/test_primitives_edges_gpu.py runs -- so that the GPU tests are not the first thing to
exercise them -- plus the merge reference's own unit cases and, for every input generator the GPU tests
use, the planted conditions they rely on (no GPU test can pass by vacuity).  No GPU needed."""
import numpy as np
import pytest

import primitives_ref as pr


# ------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize("D,n", [(1, 1), (3, 5), (63, 9), (64, 33), (65, 2), (128, 17), (300, 3)])
def test_project32_is_the_oracles_chain(oracle, D, n):
    X = pr.gen_project_input(n, D)
    E = pr.rotation(D)
    with np.errstate(invalid="ignore", over="ignore"):
        want = oracle.project(X, E)
    got = pr.project32(X, E)
    assert pr.same_bits_or_nan(got, want)
    fin = np.isfinite(want).all(axis=1)
    ref64 = pr.project64(X[fin], E)
    assert np.abs(got[fin] - ref64).max() <= 1e-4 * np.abs(ref64).max()
    if n > 2:
        assert np.isnan(want[1]).all() and not np.isfinite(want[n - 1]).all()  # the NaN row, the 3e38 row


@pytest.mark.parametrize("D", [64, 128, 256])
def test_tier_input_plants(oracle, D):
    X = pr.gen_tier_input(D)
    E = pr.rotation(D)
    ns = pr.tier_ns(D, "mid") + pr.tier_ns(D, "big")
    R = (256 // D) * 8
    assert 2048 % R == 0 and ns[3] % R == R - 1 and 2049 % R == 1       # the ragged last tiles
    assert min(ns) < 2048 <= ns[1] and max(pr.tier_ns(D, "mid")) < 65535 < 65536 <= max(ns) == pr.TIER_ROWS
    rows = [1, 2] + [n - 1 for n in ns]
    with np.errstate(invalid="ignore", over="ignore"):
        want = oracle.project(X[rows], E)
    assert np.isnan(want[0]).all()                                      # the NaN row
    assert (X[rows[1:]] == np.float32(3e38)).all() and np.isinf(want[1:]).any(axis=1).all()   # sums that overflow
    ordinary = np.ones(4096, bool)
    ordinary[[r for r in rows if r < 4096]] = False
    assert np.isfinite(X[:4096][ordinary]).all()
    assert pr.same_bits(oracle.project(X[:4096][ordinary][:64], E), pr.project32(X[:4096][ordinary][:64], E))


def test_fma_emulation_rounds_once():
    # x * y + acc lands exactly on a float32 midpoint after the float64 add; only one rounding is right
    x = np.array([[1.0 + 2.0 ** -23]], np.float32)
    y = np.array([[1.0 + 2.0 ** -23]], np.float32)          # product = 1 + 2^-22 + 2^-46
    acc = np.array([[2.0 ** 30]], np.float32)               # sum needs 77 bits
    exact = (1 + 2 ** -23) ** 2 + 2.0 ** 30                 # float64 drops the 2^-46
    got = pr._fma32(x, y, acc)
    assert got.dtype == np.float32 and got[0, 0] == np.float32(exact)
    # a tie that the dropped bits break upwards: 2^24 + 1 + tiny -> rounds up, double rounding says down
    x = np.array([[1.0 + 2.0 ** -23]], np.float32)
    y = np.array([[1.0 + 2.0 ** -23]], np.float32)
    acc = np.array([[2.0 ** 24]], np.float32)
    # exact = 2^24 + 1 + 2^-22 + 2^-46: above the midpoint 2^24 + 1 of [2^24, 2^24 + 2]
    assert pr._fma32(x, y, acc)[0, 0] == np.float32(2.0 ** 24 + 2)


def test_checked_case_plants(oracle):
    c = pr.gen_checked_case()
    with np.errstate(invalid="ignore", over="ignore"):
        Xp = oracle.project(c["X"], c["eig"])
        prod = c["X"][pr.CHECKED_OVF_QUERY][:, None].astype(np.float32) * c["eig"]
    assert np.isinf(prod).mean() > 0.5                                # overflow in the product itself
    assert not np.isfinite(Xp[pr.CHECKED_INF_QUERY]).any()
    assert not np.isfinite(Xp[pr.CHECKED_OVF_QUERY]).any()
    rest = np.ones(pr.CHECKED_NQ, bool)
    rest[[pr.CHECKED_INF_QUERY, pr.CHECKED_OVF_QUERY]] = False
    assert np.isfinite(Xp[rest]).all()
    assert pr.CHECKED_NQ >= 2048 and sum(c["bits"]) <= 256
    assert not c["X"][pr.CHECKED_ZERO_QUERY].any()


# --------------------------------------------------------------------------------------------- encoder
ENC_GRID = [
    (128, [8] * 8, 257),          # L = 16
    (8, [4, 4], 1000),            # L = 4, M = 2
    (8, [15, 1, 13, 9], 40),      # L = 2: 32768 and 8192 centroids next to 2
    (12, [6, 5, 3, 8], 300),      # generic L = 3
    (20, [6, 5, 3, 8], 300),      # generic L = 5
    (160, [6, 5, 3, 8], 64),      # generic L = 40
]


@pytest.mark.parametrize("D,bits,n", ENC_GRID, ids=[f"d{d}m{len(b)}" for d, b, _ in ENC_GRID])
def test_encode32_is_the_oracles_argmin(oracle, D, bits, n):
    rng = np.random.default_rng(D + n)
    L = D // len(bits)
    cents = [(rng.normal(size=(1 << b, L)) * 30).astype(np.float32) for b in bits]
    Xp = (rng.normal(size=(n, D)) * 30).astype(np.float32)
    Xp[0, :L] = cents[0][1]
    want = oracle.encode(Xp, cents)
    got = pr.encode32(Xp, cents)
    assert np.array_equal(got, want)
    # the float64 guard, on the reference itself
    _, m64 = pr.encode64(Xp, cents)
    d32 = pr.code_dist32(Xp, cents, got)
    assert (np.abs(d32 - m64) <= pr.sum_bound(L, m64)).all()


@pytest.mark.parametrize("L", [16, 5])
def test_encoder_planted_rows(oracle, L):
    bits = [9, 8, 8, 8, 8, 8, 8, 8] if L == 16 else [9, 5, 3, 8]
    Xp, cents, rows = pr.gen_encoder_planted(L, bits)
    want = oracle.encode(Xp, cents)   # vo_encode: `if (dist < bsf)` from bsf = FLT_MAX, VAQ.cpp:736-745
    assert np.array_equal(pr.encode32(Xp, cents), want)
    d0 = pr.sqdist32(Xp[:, :L], cents[0])
    for name in ("nan", "inf", "huge"):
        assert not np.isfinite(d0[rows[name]]).any(), name     # every distance of the row non-finite
        assert want[rows[name], 0] == 0
    assert (want[rows["huge"]] == 0).all()
    dh = [pr.sqdist32(Xp[rows["huge"]:rows["huge"] + 1, s * L:(s + 1) * L], cents[s]) for s in range(len(bits))]
    assert all(np.isinf(d).all() for d in dh)
    assert want[rows["negzero"], 0] == 5 and np.signbit(Xp[rows["negzero"], 0])
    assert want[rows["dup"], 0] == 0 and np.array_equal(cents[0][0], cents[0][511])


# ------------------------------------------------------------------------------------------ old refine
@pytest.mark.parametrize("D,R", [(1, 257), (7, 257), (128, 1), (128, 3), (128, 256), (128, 2048), (960, 257)])
def test_refine32_is_the_oracles(oracle, D, R):
    Xq, Xt, cand = pr.gen_refine_case(D, R)
    for k in sorted({1, min(R, 100), R}):
        o_lab, o_dis = oracle.refine(Xq, Xt, cand, k)
        lab, dis = pr.refine32(Xq, Xt, cand, k)
        assert pr.same_bits(dis, o_dis)
        assert np.array_equal(lab, pr.sort_tie_runs(o_lab, o_dis))
        d64 = pr.refine64_dists(Xq, Xt, lab)
        assert (np.abs(dis - d64) <= pr.sum_bound(D, d64)).all()


def test_refine_planted_conditions(oracle):
    Xq, Xt, cand = pr.gen_refine_planted()
    R = cand.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        d_huge = ((Xq[0] - Xt[pr.REFINE_HUGE]) ** 2).astype(np.float32)
        d_nan = ((Xq[0] - Xt[pr.REFINE_NAN]) ** 2).astype(np.float32)
    assert np.isinf(d_huge).all()            # the distance overflows
    assert np.isnan(d_nan).any()             # ... or is NaN
    assert (cand == pr.REFINE_HUGE).any(axis=1)[[0, 1, 2, 4]].all() and (cand == pr.REFINE_NAN).any(axis=1)[[0, 1, 2, 4]].all()
    assert (cand[pr.REFINE_EMPTY_QUERY] == -1).all()
    assert (cand[1] == pr.REFINE_TWICE).sum() == 2
    assert (cand[4, 4:-1] == -1).any() and (cand[4, 5:] >= 0).any()
    a, b = pr.REFINE_DUP
    assert np.array_equal(Xt[a], Xt[b]) and list(cand[0]).index(b) < list(cand[0]).index(a)
    for k in (100, R):
        lab, dis = pr.refine32(Xq, Xt, cand, k)
        assert lab[0, 0] == a and lab[0, 1] == b and dis[0, 0] == dis[0, 1]        # tie: smaller label first
        assert (lab[1, :2] == pr.REFINE_TWICE).all()                              # kept twice
        assert not np.isin(lab, [pr.REFINE_HUGE, pr.REFINE_NAN]).any()            # never returned
        assert (lab[pr.REFINE_EMPTY_QUERY] == -1).all() and (dis[pr.REFINE_EMPTY_QUERY] == pr.FLT_MAX).all()
        if k == R:
            assert lab[0, -1] == -1 and dis[0, -1] == pr.FLT_MAX                  # unfilled slots
        # the oracle query by query on the compacted list (vo_refine reads every label it is given)
        for q in range(cand.shape[0]):
            c = cand[q][cand[q] >= 0]
            if c.size == 0:
                continue
            o_lab, o_dis = oracle.refine(Xq[q:q + 1], Xt, c[None, :], k)
            assert pr.same_bits(dis[q:q + 1], o_dis)
            assert np.array_equal(lab[q:q + 1], pr.sort_tie_runs(o_lab, o_dis))


# ----------------------------------------------------------------------------------------------- merge
def test_merge_ref_unit_cases():
    F = pr.FLT_MAX
    # a cross-list tie at the cut: the smaller label wins, whichever list holds it
    d = np.array([[[1.0, 5.0]], [[5.0, F]]], np.float32)
    l = np.array([[[10, 40]], [[30, -1]]], np.int32)
    lab, dis = pr.merge_ref(d, l, 2)
    assert lab.tolist() == [[10, 30]] and dis.tolist() == [[1.0, 5.0]]
    # all empty
    d = np.full((3, 2, 4), F, np.float32)
    l = np.full((3, 2, 4), -1, np.int32)
    lab, dis = pr.merge_ref(d, l, 4)
    assert (lab == -1).all() and (dis == F).all()
    # k larger than the number of entries
    d = np.array([[[2.0, F, F]], [[1.0, 2.0, F]]], np.float32)
    l = np.array([[[7, -1, -1]], [[9, 3, -1]]], np.int32)
    lab, dis = pr.merge_ref(d, l, 3)
    assert lab.tolist() == [[9, 3, 7]] and dis.tolist() == [[1.0, 2.0, 2.0]]
    lab, dis = pr.merge_ref(d, l, 5)
    assert lab.tolist() == [[9, 3, 7, -1, -1]] and dis[0, 3:].tolist() == [float(F)] * 2
    # no lists at all
    lab, dis = pr.merge_ref(np.empty((0, 2, 3), np.float32), np.empty((0, 2, 3), np.int32), 3)
    assert (lab == -1).all() and (dis == F).all()
    # a poison pair (distance 0, label -1) is no entry
    lab, dis = pr.merge_ref(np.array([[[0.0, 3.0]]], np.float32), np.array([[[-1, 4]]], np.int32), 1)
    assert lab.tolist() == [[4]]


@pytest.mark.parametrize("n_lists", [1, 2, 3, 16])
@pytest.mark.parametrize("k", [1, 2, 127, 128, 129, 1024])
def test_merge_generator(n_lists, k):
    d, l = pr.gen_merge_case(n_lists, k)
    assert d.shape == (n_lists, pr.MERGE_NQ, k)
    real = l[l >= 0]
    assert real.size == np.unique(real).size and real.min() >= 1        # global distinct labels, none 0
    assert (d[l < 0] == pr.FLT_MAX).all()
    for i in range(n_lists):
        for q in range(pr.MERGE_NQ):
            f = int((l[i, q] >= 0).sum())
            assert (l[i, q, f:] == -1).all()
            key = [(d[i, q, j], l[i, q, j]) for j in range(f)]
            assert key == sorted(key)                                    # each list ascending
    assert (l[:, pr.MERGE_EMPTY_QUERY] == -1).all()
    if n_lists >= 2:
        assert pr.merge_cut_tie(d, l, k, pr.MERGE_TIE_QUERY)
        lab, dis = pr.merge_ref(d, l, k)
        assert lab[pr.MERGE_TIE_QUERY, k - 1] == l[1, pr.MERGE_TIE_QUERY, 0]   # the smaller label, from list 1
        assert l[1, pr.MERGE_TIE_QUERY, 0] < l[0, pr.MERGE_TIE_QUERY, k - 1]
    if k >= 2 and n_lists >= 2:
        fills = {int((l[i, q] >= 0).sum()) for i in range(n_lists) for q in range(pr.MERGE_NQ)}
        assert 0 in fills and len(fills) >= 2


def test_merge_generator_large_labels():
    top = 2 ** 31 - 2
    d, l = pr.gen_merge_case(3, 128, label_top=top)
    assert l.max() == top and l.dtype == np.int32
    lab, _ = pr.merge_ref(d, l, 128)
    assert lab.max() > 2 ** 31 - 2 - 4 * l.size
