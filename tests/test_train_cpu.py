"""The host half of training from raw rows (vaqhip_train_plan, vaqhip_allocate_bits, vaqhip_sym_eigen_host and the
refusals of every new entry point that needs no device), against tests/golden/train -- recorded from the reference's
own statements of VAQ.cpp:11-336 (tests/golden/train/README.md) -- and against numpy.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import train_ref as tr

EINVAL, ENOCONV = -1, -8
CASES = sorted(tr.CASES)
ROBUST = [c for c in CASES if c != "deficient"]


@pytest.fixture(scope="module")
def fixtures():
    return {name: dict(tr.load_fixture(name)) for name in CASES}


def _plan(vaqlib, fx):
    n, D, M = (int(v) for v in fx["shape"])
    return tr.train_plan(vaqlib, fx["eigenvalues"], M, float(fx["percent_var"]), int(fx["min_bits"]), int(fx["max_bits"]))


# ---- the fixtures themselves ----
@pytest.mark.parametrize("name", CASES)
def test_inputs_regenerate(fixtures, name):
    X = tr.make_inputs(name)
    assert tuple(X.shape) == tr.CASES[name][:2]
    assert tr.digest(X) == str(fixtures[name]["inputs_digest"])


@pytest.mark.parametrize("name", ROBUST)
def test_recorded_decisions_are_robust(fixtures, name):
    """Neighbouring eigenvalues differ by more than 1e-3 relative, no cumulative sum lies within 1e-3 of percent_var,
    no ratio within 1e-3 relative of a power of two: the condition under which decisions can be compared at all."""
    fx = fixtures[name]
    ev = fx["eigenvalues"][fx["sorted"]].astype(np.float64)
    assert np.all(np.diff(ev) < 0)
    assert np.min(np.abs(np.diff(ev)) / np.abs(ev[:-1])) > 1e-3
    pv = float(fx["percent_var"])
    cum = fx["cum_var"].astype(np.float64)
    # (at percent_var = 1 the LAST sum is 1 up to an ulp by construction: every other one is still checked, and
    # test_where_the_last_lower_bound_moves_the_bits covers the decision that hangs on the last)
    assert np.min(np.abs((cum if pv < 1 else cum[:-1]) - pv)) > 1e-3
    H = int(fx["highest_subs"])
    var = fx["var_per_subs"].astype(np.float64)
    for i in range(H - 1):
        ratio = var[i] / var[i + 1]
        for p in (2.0 ** np.floor(np.log2(ratio)), 2.0 ** np.ceil(np.log2(ratio))):
            assert abs(ratio / p - 1) > 1e-3, (name, i, ratio)


def test_every_case_shows_what_it_names(fixtures):
    assert int(fixtures["balance_kept"]["swaps_kept"]) >= 1
    assert int(fixtures["balance_undone"]["swaps_kept"]) == 0
    fx = fixtures["percent"]
    assert int(fx["highest_subs"]) < int(fx["shape"][2])
    assert float(fx["cum_var"][0]) > float(fx["percent_var"])  # ... so lb[0] is 0
    assert 1 < int(fixtures["percent_two"]["highest_subs"]) < 4
    n, D, _ = fixtures["sampled"]["shape"]
    assert 1000 * D < n and len(tr.sample_rows(int(n), int(D))) == 1000 * D
    assert tr.make_inputs("bytes").dtype == np.uint8
    ev = fixtures["deficient"]["eigenvalues"]
    assert np.sum(np.abs(ev) < 1e-4 * np.max(ev)) >= 2 and fixtures["deficient"]["var_per_subs"].min() < 1e-6


# ---- the plan ----
@pytest.mark.parametrize("name", CASES)
def test_plan_equals_the_reference(vaqlib, fixtures, name):
    fx = fixtures[name]
    got = _plan(vaqlib, fx)
    assert isinstance(got, dict), got
    H = int(fx["highest_subs"])
    assert got["highest"] == H
    if name == "deficient":
        # zero eigenvalues come in an order of the solver's own rounding: compared are the decisions taken from the
        # 6 - 1 non-zero ones (README): the leading columns, the swaps kept, highest_subs, the first two variances
        nz = 5
        assert np.array_equal(got["sorted"][:nz], fx["sorted"][:nz])
        assert got["swaps_kept"] == int(fx["swaps_kept"])
        assert np.array_equal(got["var"][:2].view(np.uint32), fx["var_per_subs"][:2].view(np.uint32))
        assert np.array_equal(got["k"][:1], fx["k"][:1])
        return
    assert np.array_equal(got["sorted"], fx["sorted"])
    assert np.array_equal(got["order"], fx["balanced"])
    assert got["swaps_kept"] == int(fx["swaps_kept"])
    assert np.array_equal(got["var"].view(np.uint32), fx["var_per_subs"].view(np.uint32))
    assert np.array_equal(got["cum"].view(np.uint32), fx["cum_var"].view(np.uint32))
    assert np.array_equal(got["k"], fx["k"])
    pv = np.float32(fx["percent_var"])
    assert np.array_equal(got["lb"], np.where(fx["cum_var"][:H] <= pv, int(fx["min_bits"]), 0))


def test_plan_long_subspaces_take_eigens_packet_order(vaqlib):
    """L = 24 and 20: segments that start on and off a 32-byte boundary, against a float32 restatement in numpy."""
    rng = np.random.Generator(np.random.PCG64(5))

    def eigen_sum(v, off, size):
        x = v[off:off + size]
        start = min((8 - off % 8) % 8, size)
        n1, n2 = (size - start) // 8 * 8, (size - start) // 16 * 16
        if n1 == 0:
            res = x[0]
            for e in x[1:]:
                res = np.float32(res + e)
            return res
        a0 = x[start:start + 8].copy()
        if n1 > 8:
            a1 = x[start + 8:start + 16].copy()
            for i in range(start + 16, start + n2, 16):
                a0 = a0 + x[i:i + 8]
                a1 = a1 + x[i + 8:i + 16]
            a0 = a0 + a1
            if n1 > n2:
                a0 = a0 + x[start + n2:start + n2 + 8]
        res = np.float32(np.float32(np.float32(a0[0] + a0[4]) + np.float32(a0[2] + a0[6])) +
                         np.float32(np.float32(a0[1] + a0[5]) + np.float32(a0[3] + a0[7])))
        for e in list(x[:start]) + list(x[start + n1:]):
            res = np.float32(res + e)
        return res

    for D, M in ((96, 4), (80, 4), (36, 3)):
        L = D // M
        ev = np.sort(rng.random(D).astype(np.float32) + np.float32(0.01))[::-1].copy()
        ev[:L] += np.float32(50.0)  # (the first swap would leave the sums unsorted only by accident: keep it simple)
        got = tr.train_plan(vaqlib, ev, M, 1.0, 1, 8)
        v = ev[got["order"]]
        v = (v / eigen_sum(v, 0, D)).astype(np.float32)
        want = np.array([eigen_sum(v, s * L, L) for s in range(M)], np.float32)
        assert np.array_equal(got["var"].view(np.uint32), want.view(np.uint32)), (D, M)


def test_plan_refusals(vaqlib):
    ev = np.linspace(4, 1, 8).astype(np.float32)
    assert tr.train_plan(vaqlib, ev, 3, 1.0, 1, 8) == EINVAL          # D % M
    assert tr.train_plan(vaqlib, ev, 4, 1.0, 5, 4) == EINVAL          # min > max
    assert tr.train_plan(vaqlib, ev, 4, 1.0, 1, 16) == EINVAL         # max_bits > VAQHIP_MAX_BITS
    big = np.ones(256, np.float32)
    assert tr.train_plan(vaqlib, big, 256, 1.0, 1, 8) == EINVAL       # M > VAQHIP_MAX_SUBSPACES
    bad = ev.copy()
    bad[3] = np.nan
    assert tr.train_plan(vaqlib, bad, 4, 1.0, 1, 8) == EINVAL
    bad[3] = np.inf
    assert tr.train_plan(vaqlib, bad, 4, 1.0, 1, 8) == EINVAL
    assert tr.train_plan(vaqlib, -ev, 4, 1.0, 1, 8) == EINVAL         # non-positive sum
    assert tr.train_plan(vaqlib, np.zeros(8, np.float32), 4, 1.0, 1, 8) == EINVAL
    assert b"sum" in vaqlib.vaqhip_last_error()
    assert vaqlib.vaqhip_train_plan(None, 8, 4, 1.0, 1, 8, None, None, None, None, None, None, None, None) == EINVAL


def test_plan_k_is_clamped(vaqlib):
    ev = np.array([1e30, 1.0, 1e-3, 1e-5], np.float32)
    got = tr.train_plan(vaqlib, ev, 4, 1.0, 1, 8)
    assert got["k"].tolist()[0] == 1 << 30 and np.all(got["k"] >= 0)
    up = tr.train_plan(vaqlib, np.array([1.0, 2.0, 3.0, 4.5], np.float32), 2, 1.0, 1, 8)
    assert up["sorted"].tolist() == [3, 2, 1, 0]
    tie = tr.train_plan(vaqlib, np.array([2.0, 5.0, 2.0, 5.0], np.float32), 4, 1.0, 1, 8)
    assert tie["sorted"].tolist() == [1, 3, 0, 2]  # equal values by ascending column


# ---- the allocation ----
def _random_instances():
    rng = np.random.Generator(np.random.PCG64(2024))
    out = []
    while len(out) < 200:
        H = int(rng.integers(1, 7))
        max_bits = int(rng.integers(1, 9))
        c = np.sort(rng.random(H).astype(np.float32))[::-1].copy()
        if rng.random() < 0.3:  # ties: equal coefficients
            c[:] = c[0]
        lb = rng.integers(0, min(max_bits, 3) + 1, H).tolist()
        k = [int(2 ** rng.integers(0, 4)) if rng.random() < 0.8 else 0 for _ in range(H - 1)]
        budget = int(rng.integers(0, 25))
        out.append((c, lb, max_bits, k, budget))
    return out


def test_allocation_equals_brute_force(vaqlib, fixtures):
    inst = _random_instances()
    for name in CASES:
        fx = fixtures[name]
        H = int(fx["highest_subs"])
        lb = np.where(fx["cum_var"][:H] <= np.float32(fx["percent_var"]), int(fx["min_bits"]), 0).tolist()
        inst.append((fx["var_per_subs"][:H], lb, int(fx["max_bits"]), fx["k"].tolist(), int(fx["bit_budget"])))
    feasible = 0
    for c, lb, max_bits, k, budget in inst:
        want = tr.brute_force_bits(c, lb, max_bits, k, budget)
        got = tr.allocate_bits(vaqlib, c, lb, max_bits, k, budget)
        if want is None:
            assert got == EINVAL, (c, lb, max_bits, k, budget, got)
            continue
        feasible += 1
        assert got[0] == want[0] and got[1] == want[1], (c, lb, max_bits, k, budget, got, want)
    assert feasible >= 60


LAST_LB_MOVES_BITS = {"balance_undone", "deficient"}


@pytest.mark.parametrize("name", [c for c in CASES if tr.CASES[c][3] >= 1.0])
def test_where_the_last_lower_bound_moves_the_bits(vaqlib, fixtures, name):
    """At percent_var = 1, lb[M - 1] is min_bits or 0 by whether a float sum that is 1 up to an ulp exceeds 1: no solver's
    eigenvalues make that robust, and it MAY change the allocation.  This names the fixtures on which it does
    (the smallest subspace would otherwise get 0 bits); tests/test_train_gpu.py takes that one bound from the plan of
    the device's own eigenvalues instead of comparing it."""
    fx = fixtures[name]
    H = int(fx["highest_subs"])
    lb = np.where(fx["cum_var"][:H] <= np.float32(fx["percent_var"]), int(fx["min_bits"]), 0)
    got = []
    for last in (0, int(fx["min_bits"])):
        lb[-1] = last
        got.append(tr.allocate_bits(vaqlib, fx["var_per_subs"][:H], lb, int(fx["max_bits"]), fx["k"], int(fx["bit_budget"])))
    assert not isinstance(got[0], int) and not isinstance(got[1], int)
    assert (got[0] != got[1]) == (name in LAST_LB_MOVES_BITS), got


def _milp_optimum(c, lb, max_bits, k, budget):
    so = pytest.importorskip("scipy.optimize")
    H = len(c)
    rows, lo, hi = [np.ones(H)], [budget], [budget]
    for i in range(H - 1):
        r = np.zeros(H)
        r[i], r[i + 1] = 1, -1
        rows.append(r)
        lo.append(-np.inf)
        hi.append(k[i])
    res = so.milp(-np.asarray(c, np.float64), constraints=so.LinearConstraint(np.array(rows), lo, hi),
                  integrality=np.ones(H), bounds=so.Bounds(np.asarray(lb, float), np.full(H, float(max_bits))))
    return -res.fun if res.success else None


def test_allocation_optimum_equals_milp(vaqlib):
    pytest.importorskip("scipy")
    inst = _random_instances()
    rng = np.random.Generator(np.random.PCG64(77))
    for M, B, lo, hi in ((16, 128, 1, 12), (32, 256, 2, 13)):
        ev = np.sort((rng.random(M) ** 3).astype(np.float32) + np.float32(1e-3))[::-1]
        c = (ev / ev.sum()).astype(np.float32)
        k = [tr_next_pow2(float(np.float32(c[i] / c[i + 1]))) for i in range(M - 1)]
        inst.append((c, [lo] * M, hi, k, B))
    checked = 0
    for c, lb, max_bits, k, budget in inst:
        want = _milp_optimum(c, lb, max_bits, k, budget)
        got = tr.allocate_bits(vaqlib, c, lb, max_bits, k, budget)
        if want is None:
            assert got == EINVAL
            continue
        checked += 1
        assert abs(got[1] - want) <= 1e-9 * max(abs(want), 1e-300), (c, lb, max_bits, k, budget, got, want)
        bits = got[0]
        assert sum(bits) == budget and all(lb[i] <= bits[i] <= max_bits for i in range(len(bits)))
        assert all(bits[i] - bits[i + 1] <= k[i] for i in range(len(bits) - 1))
    assert checked >= 62


def tr_next_pow2(x: float) -> int:
    return 0 if x == 0 else max(int(min(2.0 ** np.floor(np.log2(abs(x))), 2.0 ** 30)), 0)


def test_allocation_infeasible(vaqlib):
    c = np.array([0.5, 0.3, 0.2], np.float32)
    assert tr.allocate_bits(vaqlib, c, [1, 1, 1], 4, [8, 8], 13) == EINVAL      # budget above H * max_bits
    assert tr.allocate_bits(vaqlib, c, [4, 2, 1], 4, [0, 0], 7) == EINVAL       # k = 0 chain against the lower bounds
    assert tr.allocate_bits(vaqlib, c, [2, 2, 2], 4, [8, 8], 5) == EINVAL       # budget below the lower bounds
    assert tr.allocate_bits(vaqlib, c, [1, 1, 1], 4, [8, 8], 12)[0] == [4, 4, 4]
    assert tr.allocate_bits(vaqlib, np.array([0.5, np.nan, 0.2], np.float32), [1, 1, 1], 4, [8, 8], 6) == EINVAL
    assert tr.allocate_bits(vaqlib, c, [1, 5, 1], 4, [8, 8], 6) == EINVAL       # lb above max_bits
    assert vaqlib.vaqhip_allocate_bits(None, 3, None, 4, None, 6, None, None) == EINVAL
    tie = tr.allocate_bits(vaqlib, np.array([0.25] * 4, np.float32), [0] * 4, 8, [8, 8, 8], 10)
    assert tie[0] == [8, 2, 0, 0]  # the lexicographically greatest of the optima


# ---- the host Jacobi ----
@pytest.fixture(scope="module")
def matrices():
    return tr.eigen_matrices()


EIGEN_CASES = ["d1", "d2", "d3", "d5", "d64", "diagonal", "repeated", "zero", "graded"]


@pytest.mark.parametrize("name", EIGEN_CASES)
def test_host_jacobi_invariants(vaqlib, matrices, name):
    """Residual and orthogonality at most 8 x what numpy.linalg.eigh (double) leaves on the same matrix (measured here,
    per case; where eigh leaves exactly 0 the bound is 0), eigenvalues against eigh's relative to
    the 2-norm."""
    A = matrices[name]
    D = A.shape[0]
    rc, values, vectors, sweeps = tr.sym_eigen_host(vaqlib, A)
    assert rc == 0 and 0 <= sweeps <= tr.MAX_SWEEPS
    w, Vh = np.linalg.eigh(A)
    norm = max(float(np.max(np.abs(w))), 0.0)
    e_res, e_orth = tr.eigh_quality(A, w, Vh)
    res, orth = tr.eigh_quality(A, values, vectors)
    eps = np.finfo(np.float64).eps
    print(f"{name}: D={D} sweeps={sweeps} residual ours {res:.3e} eigh {e_res:.3e}; orthogonality ours {orth:.3e} "
          f"eigh {e_orth:.3e}")
    # 8 x eigh's own figure; where eigh leaves exactly 0 (d1, diagonal, zero) so must ours
    assert res <= 8 * e_res
    assert orth <= 8 * e_orth
    assert np.all(np.diff(values) <= 0)
    assert np.max(np.abs(values - w[::-1])) <= 8 * D * eps * norm
    if name in ("diagonal", "zero", "d1"):
        assert sweeps == 0


@pytest.mark.parametrize("name", EIGEN_CASES)
def test_host_jacobi_equals_its_numpy_restatement(vaqlib, matrices, name):
    A = matrices[name]
    rc, values, vectors, sweeps = tr.sym_eigen_host(vaqlib, A)
    r_values, r_vectors, r_sweeps = tr.jacobi_ref(A)
    assert rc == 0 and sweeps == r_sweeps
    assert np.array_equal(values.view(np.uint64), r_values.view(np.uint64))
    assert np.array_equal(vectors.view(np.uint64), np.ascontiguousarray(r_vectors).view(np.uint64))


def test_host_jacobi_order_and_signs(vaqlib, matrices):
    rc, values, vectors, _ = tr.sym_eigen_host(vaqlib, matrices["diagonal"])  # diag 4 -1 9 .5 9 2
    assert rc == 0 and values.tolist() == [9.0, 9.0, 4.0, 2.0, 0.5, -1.0]
    assert np.argmax(vectors, axis=0).tolist() == [2, 4, 0, 5, 3, 1]  # equal values by ascending column
    assert np.array_equal(np.abs(vectors).sum(axis=0), np.ones(6))
    for name in ("d5", "d64", "repeated"):
        _, _, vec, _ = tr.sym_eigen_host(vaqlib, matrices[name])
        big = np.argmax(np.abs(vec), axis=0)
        assert np.all(vec[big, np.arange(vec.shape[0])] > 0)
    # a tie of magnitudes: (1, -1) / sqrt 2 -- the first component decides
    _, _, vec, _ = tr.sym_eigen_host(vaqlib, np.array([[1.0, -1.0], [-1.0, 1.0]]))
    assert vec[0, 0] > 0 and vec[1, 0] < 0


def test_host_jacobi_refusals(vaqlib):
    A = np.eye(3)
    A[1, 2] = np.nan
    assert tr.sym_eigen_host(vaqlib, A)[0] == EINVAL
    A[1, 2] = np.inf
    assert tr.sym_eigen_host(vaqlib, A)[0] == EINVAL
    out = np.zeros(9)
    assert vaqlib.vaqhip_sym_eigen_host(None, 3, tr._p(out), tr._p(out), None) == EINVAL
    assert vaqlib.vaqhip_sym_eigen_host(tr._p(out), 0, tr._p(out), tr._p(out), None) == EINVAL
    assert vaqlib.vaqhip_sym_eigen_host(tr._p(out), 4097, tr._p(out), tr._p(out), None) == EINVAL


# ---- refusals of the device entry points, all before a device is touched ----
def test_device_entry_refusals(vaqlib):
    X = np.zeros((4, 8), np.float32)
    cov = np.zeros((8, 8))
    hi = C.c_int(0)
    bits = np.zeros(4, np.int32)
    eig = np.zeros((8, 8), np.float32)
    p = tr._p
    for fn in (vaqlib.vaqhip_train_moment, vaqlib.vaqhip_train_moment_u8):
        assert fn(0, None, 4, 8, p(cov), None) == EINVAL
        assert fn(0, p(X), 4, 8, None, None) == EINVAL
        assert fn(0, p(X), 0, 8, p(cov), None) == EINVAL
        assert fn(0, p(X), 1 << 31, 8, p(cov), None) == EINVAL
        assert fn(0, p(X), 4, 0, p(cov), None) == EINVAL
        assert fn(0, p(X), 4, 4097, p(cov), None) == EINVAL
    for fn in (vaqlib.vaqhip_train_moment_device, vaqlib.vaqhip_train_moment_u8_device):
        assert fn(0, None, 4, 8, p(cov), None, None) == EINVAL
        assert fn(0, p(X), 4, 4097, p(cov), None, None) == EINVAL
    assert vaqlib.vaqhip_refiner_train_moment(None, p(cov), None) == EINVAL
    assert vaqlib.vaqhip_refiner_train_rotation(None, 4, 16, 1, 8, 1.0, p(eig), None, p(bits), C.byref(hi)) == EINVAL
    assert vaqlib.vaqhip_sym_eigen_device(0, None, 8, p(cov), p(cov), None, None) == EINVAL
    assert vaqlib.vaqhip_sym_eigen_device(0, p(cov), 0, p(cov), p(cov), None, None) == EINVAL
    for fn in (vaqlib.vaqhip_train_rotation, vaqlib.vaqhip_train_rotation_u8):
        args = lambda **kw: [kw.get("dev", 0), kw.get("X", p(X)), kw.get("n", 4), kw.get("D", 8), kw.get("M", 4),  # noqa: E731
                             kw.get("B", 16), kw.get("lo", 1), kw.get("hi", 8), kw.get("pv", 1.0), kw.get("eig", p(eig)),
                             None, kw.get("bits", p(bits)), C.byref(hi)]
        assert fn(*args(X=None)) == EINVAL
        assert fn(*args(eig=None)) == EINVAL
        assert fn(*args(bits=None)) == EINVAL
        assert fn(*args(n=0)) == EINVAL
        assert fn(*args(n=1 << 31)) == EINVAL
        assert fn(*args(D=4097)) == EINVAL
        assert fn(*args(M=3)) == EINVAL
        assert fn(*args(lo=9)) == EINVAL
        assert fn(*args(hi=16)) == EINVAL
        assert fn(*args(B=-1)) == EINVAL
    assert vaqlib.vaqhip_train_rotation_device(0, None, 4, 8, 4, 16, 1, 8, 1.0, p(eig), None, p(bits), C.byref(hi), None) == EINVAL
    assert vaqlib.vaqhip_train_rotation_u8_device(0, p(X), 4, 8, 3, 16, 1, 8, 1.0, p(eig), None, p(bits), C.byref(hi), None) == EINVAL
    assert vaqlib.vaqhip_last_train_timing(None) == EINVAL


def test_python_surface():
    import vaq_amd
    for name in ("train_rotation", "train", "last_train_timing"):
        assert callable(getattr(vaq_amd, name)) and name in vaq_amd.__all__
    assert callable(vaq_amd.VaqRefiner.train_rotation) and callable(vaq_amd.VaqRefiner.train)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        vaq_amd.train_rotation(np.zeros((4, 8), np.float32), 3, 16, 1, 8)
    assert e.value.code == EINVAL
