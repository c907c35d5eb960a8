"""The k-means of VAQ::clusterTI(true) on the CPU: tests/kmeans_ref.py (a NumPy restatement of
KMeans::staticFitCodebook, KMeans.hpp:487-652) against the fixtures recorded from the reference itself
(tests/golden/kmeans/README.md)."""
import numpy as np
import pytest

import fast_ref as fr
import kmeans_ref as kr

CASES = list(kr.CASES)
# the one fixture on which the summation order of squaredNorm decides centres (see the README)
ORDER_CASE = "n40000_s4_l16_t100"


@pytest.fixture(scope="module")
def fits():
    """Every case fitted once by the restatement, shared by the tests below."""
    out = {}
    for name in CASES:
        N, seg, L, T, ncent, M = kr.CASES[name]
        codes, cents = kr.make_inputs(name)
        out[name] = (codes, cents) + kr.fit_codebook(codes, cents, seg, T)
    return out


@pytest.mark.parametrize("name", CASES)
def test_inputs_are_the_recorded_ones(name):
    codes, cents = kr.make_inputs(name)
    fx = kr.load_fixture(name)
    assert tuple(int(v) for v in fx["shape"]) == kr.CASES[name]
    assert int(fx["max_iter"]) == kr.MAX_ITER
    assert str(fx["inputs_digest"]) == kr.digest(codes, cents), "numpy no longer generates the recorded inputs"


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(fits, name):
    fx = kr.load_fixture(name)
    _, _, means, iters, nan = fits[name]
    kr.assert_centres_equal(means, fx["centres"], name)
    assert iters == int(fx["iterations"])
    assert np.array_equal(nan, fx["nan_rows"])
    assert np.array_equal(np.isnan(fx["centres"]).any(axis=1), fx["nan_rows"])


def test_fixtures_cover_both_endings():
    """At least one run that converges before the cap, one that runs to it with NaN centres; both branches of
    the sampling; an odd row count."""
    fxs = {n: kr.load_fixture(n) for n in CASES}
    assert any(int(f["iterations"]) < kr.MAX_ITER and not f["nan_rows"].any() for f in fxs.values())
    assert any(int(f["iterations"]) == kr.MAX_ITER and f["nan_rows"].any() for f in fxs.values())
    for n, f in fxs.items():  # a NaN centre never compares equal: the loop cannot stop early
        assert not f["nan_rows"].any() or int(f["iterations"]) == kr.MAX_ITER, n
    sampled = [n for n, c in kr.CASES.items() if c[0] > kr.ROWS_PER_CENTRE * c[3]]
    assert sampled and len(sampled) < len(CASES)
    assert any(min(c[0], kr.ROWS_PER_CENTRE * c[3]) % 2 == 1 for c in kr.CASES.values())


def test_summation_order_is_pinned_by_data(fits):
    """Eigen's order and the sequential one give different centres on this fixture, and the reference's are
    Eigen's: the order of squaredNorm is not a free choice."""
    N, seg, L, T, ncent, M = kr.CASES[ORDER_CASE]
    codes, cents = fits[ORDER_CASE][:2]
    seq, _, _ = kr.fit_codebook(codes, cents, seg, T, order="sequential")
    want = kr.load_fixture(ORDER_CASE)["centres"]
    assert not np.array_equal(seq.view(np.uint32), want.view(np.uint32))
    kr.assert_centres_equal(fits[ORDER_CASE][2], want, ORDER_CASE)


def test_pruned_assignment_equals_the_full_one():
    """assign() evaluates the float32 distance only for centres a float64 estimate cannot rule out."""
    rng = np.random.default_rng(5)
    for d in (3, 8, 20, 40, 64):
        base = rng.normal(size=(40, d)).astype(np.float32)
        X = base[rng.integers(0, 40, 3000)]
        means = base[rng.integers(0, 40, 33)].copy()  # many exact duplicates: ties go to the first
        means[7] = np.nan
        for order in ("eigen", "sequential"):
            assert np.array_equal(kr.assign(X, means, order), kr.assign_full(X, means, order)), (d, order)


@pytest.mark.parametrize("n,r", [(1, 1), (2, 2), (37, 37), (1000, 10), (100000, 4000)])
def test_permutation_head(n, r):
    """the sparse form against the whole permutation, and against the reference's own (FAST fixture)"""
    assert np.array_equal(kr.permutation_head(n, r), fr.random_permutation(n)[:r])


def test_permutation_head_against_recorded():
    """... and against the reference's own randomPermutation (recorded for FAST)"""
    import os
    fx = np.load(os.path.join(os.path.dirname(kr.GOLDEN), "fast", "random_permutation.npz"))
    assert np.array_equal(kr.permutation_head(37, 37), fx["perm37"])
    assert np.array_equal(kr.permutation_head(1000, 1000), fx["perm1000"])
    assert np.array_equal(kr.permutation_head(100000, 4000), fx["perm100000_head"])
