"""The first-round primitives (vaq_front.hip, vaq_codes.hip, vaq_merge.hip) at their launch-shape edges: the projection's three
kernels on both sides of their row thresholds, CreateLUT's small-codebook branch in every reduction
order, the encoder's row tiles, chunk loops and non-finite rows, the old refine on continuous data, and
the k-min merge at every fold count, fill level and stride.

Every primary comparison is on bit patterns (distances, tables) or exact equality (codes, labels),
against the exact numpy references of tests/primitives_ref.py and the compiled oracle; the float64
bounds derived in primitives_ref.py come on top as a second guard.  tests/test_primitives_ref_cpu.py
pins those references to the oracle and asserts every planted condition without a GPU."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import primitives_ref as pr
from helpers import assert_topk_matches

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2


def plain_index(bits, cents, eig=None, codes=None, seq=False):
    import vaq_amd
    v = vaq_amd.VaqHip(sequential_sum=seq)
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = cents
    v.mEigenVectors = eig
    v.mCodebook = codes
    return v


def gauss_cents(rng, bits, L, scale=30.0):
    return [(rng.normal(size=(1 << b, L)) * scale).astype(np.float32) for b in bits]


def oracle_project_mt(oracle, X, E, threads=8):
    """oracle.project over row blocks in threads (rows are independent; ctypes drops the GIL)."""
    n = X.shape[0]
    if n < 4 * threads:
        with np.errstate(invalid="ignore", over="ignore"):
            return oracle.project(X, E)
    cuts = np.linspace(0, n, threads + 1).astype(np.int64)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda i: oracle.project(X[cuts[i]:cuts[i + 1]], E), range(threads)))
    return np.concatenate(parts)


# ====================================================================================== projection ==
@pytest.fixture(scope="module")
def tier_reference(oracle):
    """pr.gen_tier_input(D) and the oracle's product of it, kept for ONE D at a time (the cases of a D run
    back to back) and dropped with the module."""
    cache = {}

    def get(D):
        if D not in cache:
            cache.clear()
            X = pr.gen_tier_input(D)
            E = pr.rotation(D)
            want = oracle_project_mt(oracle, X, E)
            want.setflags(write=False)
            X.setflags(write=False)
            cache[D] = (X, E, want)
        return cache[D]

    yield get
    cache.clear()


@pytest.mark.parametrize("tier", ["mid", "big"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_project_tiers_both_sides_of_each_threshold(vaqlib, tier_reference, D, tier):
    """launch_project: project_kernel below 2048 rows, project_tile_kernel<D, 8> from 2048 (the tier a
    10 k-query batch takes), <D, 16> from 65536.  R = (256 / D) * 8 rows per workgroup divides 2048, so
    n = 2049 leaves the middle tier's last tile one row and n = 2048 + R - 1 leaves it R - 1.  Every output
    is one fma chain over the inner index ascending: bit for bit the oracle's, the NaN row and the
    overflowing rows included (tests/test_primitives_ref_cpu.py::test_tier_input_plants checks the input)."""
    X, E, want = tier_reference(D)
    assert np.isnan(want[1]).all() and np.isinf(want[2]).any()
    L = D // 8
    v = plain_index([8] * 8, gauss_cents(np.random.default_rng(1), [8] * 8, L), eig=E)
    for n in pr.tier_ns(D, tier):
        got = v.project(X[:n])
        assert np.isinf(want[n - 1]).any()
        bad = np.nonzero(~((got.view(np.uint32) == want[:n].view(np.uint32)) | (np.isnan(got) & np.isnan(want[:n]))).all(axis=1))[0]
        assert bad.size == 0, f"D={D} n={n}: {bad.size} rows differ, first {bad[:5]}, last {bad[-5:]}"
        fin = np.isfinite(want[:n]).all(axis=1)
        ref64 = pr.project64(X[:n][fin], E)
        assert np.abs(got[fin] - ref64).max() <= 1e-4 * np.abs(ref64).max()


@pytest.mark.parametrize("n", [1, 2049])
@pytest.mark.parametrize("D", [1, 3, 63, 65, 300, 1024])
def test_project_one_row_kernel_any_width(vaqlib, oracle, D, n):
    """project_kernel for the D the tiled kernels do not take, at one row and past the tile threshold:
    a thread loop over the columns (D > 256) and a partly idle last wave (D = 1, 3, 63, 65).  D = 1024
    is accepted by index creation (M = 4, L = 256).  D < 4 or odd needs an index whose M may be no
    multiple of 4: the sequential-sum one (M = D); vaqhip_project is the same unchecked launch."""
    X = pr.gen_project_input(n, D)
    E = pr.rotation(D)
    if D in (300, 1024):
        v = plain_index([1] * 4, gauss_cents(np.random.default_rng(2), [1] * 4, D // 4), eig=E)
    else:
        v = plain_index([1] * D, gauss_cents(np.random.default_rng(2), [1] * D, 1), eig=E, seq=True)
    got = v.project(X)
    want = oracle_project_mt(oracle, X, E)
    assert pr.same_bits_or_nan(got, want)
    if n * D * D <= 5e7:
        assert pr.same_bits_or_nan(got, pr.project32(X, E))
    fin = np.isfinite(want).all(axis=1)
    if fin.any():
        ref64 = pr.project64(X[fin], E)
        assert np.abs(got[fin] - ref64).max() <= 1e-4 * np.abs(ref64).max()
    if n > 2:
        assert np.isnan(got[1]).all()
        if D >= 63:  # (3e38 times one or three entries of a rotation stays finite)
            assert not np.isfinite(got[n - 1]).all()


@pytest.mark.parametrize("with_eig", [True, False], ids=["rotated", "identity"])
def test_checked_projection_inside_the_tile_kernel(vaqlib, oracle, with_eig):
    """BitVecEngine::ProjectOnEigenVectors(Z, withChecking = true) (BitVecEngine.hpp:53-71, called by
    queryLUT at :1226) with 2048 + 5 queries of D = 64: project_tile_kernel<64, 8> with `checked` set.
    A query holding an inf and one whose products overflow come out non-finite in every coordinate, so
    both are answered as the zero vector; every other query equals the oracle's queryLUT.  The identity
    form (no mEigenVectors: project_kernel's E == nullptr branch) zeroes a row with a non-finite
    component and leaves the finite 3e38 row alone -- its distances overflow and nothing is admitted."""
    c = pr.gen_checked_case()
    D, N, bits, nq, k = c["D"], c["N"], c["bits"], pr.CHECKED_NQ, 10
    cent = np.zeros((256, D), np.float32)
    cent[:16] = c["cent"]
    eig = c["eig"] if with_eig else None
    X = c["X"]
    with np.errstate(invalid="ignore", over="ignore"):
        Xp = oracle.project(X, eig if with_eig else np.eye(D, dtype=np.float32))
    Xc = np.where(np.isfinite(Xp), Xp, np.float32(0)).astype(np.float32)
    v = plain_index(bits, [np.ascontiguousarray(cent[: 1 << b, d:d + 1]) for d, b in enumerate(bits)], eig=eig,
                    codes=c["codes"], seq=True)
    o_lab = np.empty((nq, k), np.int32)
    o_dis = np.empty((nq, k), np.float32)
    for i in range(nq):
        o_lab[i], o_dis[i] = oracle.query_lut_1d(Xc[i], bits, cent, c["codes"], k)
    with np.errstate(invalid="ignore", over="ignore"):
        ad = pr.seq_all_dists(Xc, bits, cent, c["codes"])
    a = v.search(X, k)
    lab, dis = a.labels.reshape(nq, k), a.distances.reshape(nq, k)
    assert_topk_matches(lab, dis, o_lab, o_dis, ad, what=f"checked projection, eig={with_eig}")
    z = pr.CHECKED_ZERO_QUERY
    assert (lab[z] >= 0).all()
    for q in [pr.CHECKED_INF_QUERY] + ([pr.CHECKED_OVF_QUERY] if with_eig else []):
        assert np.array_equal(lab[q], lab[z]) and pr.same_bits(dis[q], dis[z]), q
    if not with_eig:
        assert (lab[pr.CHECKED_OVF_QUERY] == -1).all() and (dis[pr.CHECKED_OVF_QUERY] == pr.FLT_MAX).all()


# ================================================================= CreateLUT, small-codebook branch ==
@pytest.mark.parametrize("nq", [9, 17])
@pytest.mark.parametrize("bits", [[1, 2, 2, 1], [2, 3, 1, 2]], ids=["b1221", "b2312"])
@pytest.mark.parametrize("D", [4, 8, 16, 12, 64])
def test_small_codebook_lut_every_reduction_order(vaqlib, oracle, D, bits, nq):
    """Subspaces of fewer than 8 centroids restate fvec_L2sqr_ny (utils/Math.hpp:147-171): L = 1, 2, 4
    have their own reduction order, L = 3 and 16 the sequential one.  bits [2, 3, 1, 2] puts an 8-centroid
    subspace (the fma branch) into the same table, with max(bits) not the first subspace's.  9 queries take
    the per-query kernel for every subspace.  17 queries of bits [2, 3, 1, 2] take the batched kernel for
    the 8-centroid subspace followed by the per-query one with `only_small` for the others; with bits
    [1, 2, 2, 1] no codebook reaches 8 centroids and 17 queries take the plain per-query kernel as 9 do.
    Then one search, so that the scan reads those tables too."""
    L = D // 4
    rng = np.random.default_rng(100 * D + sum(bits) + nq)
    cents = gauss_cents(rng, bits, L)
    codes = np.stack([rng.integers(0, 1 << b, 700) for b in bits], 1).astype(np.uint16)
    E = pr.rotation(D)
    X = (rng.normal(size=(nq, D)) * 30).astype(np.float32)
    v = plain_index(bits, cents, eig=E, codes=codes)
    Xp = oracle.project(X, E)
    want = np.stack([oracle.create_lut(Xp[q], cents, max(bits)) for q in range(nq)])
    got = v.build_lut(X)
    assert pr.same_bits(got, want), f"L={L}: {(got.view(np.uint32) != want.view(np.uint32)).sum()} entries differ"
    k = 5
    o_lab, o_dis = oracle.search(Xp, cents, codes, k, max_bits=max(bits), projected=True)
    ad = np.stack([oracle.all_dists(want[q], codes) for q in range(nq)])
    a = v.search(X, k)
    assert_topk_matches(a.labels.reshape(nq, k), a.distances.reshape(nq, k), o_lab, o_dis, ad, what=f"L={L} bits={bits}")


# ========================================================================================= encoder ==
def encode_both(v, Xp):
    """(host form, device form) codes of rows already in PCA space."""
    import torch
    v.encode(Xp, projected=True)
    host = np.array(v.mCodebook)
    dev = v.encode_device(torch.from_numpy(Xp).cuda(), projected=True).cpu().numpy().view(np.uint16)
    return host, dev


def assert_encoder_guard(Xp, cents, codes, L):
    _, m64 = pr.encode64(Xp, cents)
    d32 = pr.code_dist32(Xp, cents, codes)
    ok = np.abs(d32.astype(np.float64) - m64) <= pr.sum_bound(L, m64)
    assert ok.all(), f"float64 guard: {(~ok).sum()} codes are not a minimum"


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_encode_row_tile_edges(vaqlib, oracle, n):
    """One row per thread in tiles of 256: one row, one short of a tile, a full tile, one over."""
    rng = np.random.default_rng(n)
    bits, L = [8] * 8, 16
    cents = gauss_cents(rng, bits, L)
    Xp = (rng.normal(size=(n, 128)) * 30).astype(np.float32)
    want = oracle.encode(Xp, cents)
    assert np.array_equal(want, pr.encode32(Xp, cents))
    host, dev = encode_both(plain_index(bits, cents), Xp)
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert_encoder_guard(Xp, cents, host, L)


def test_encode_chunk_loop_past_2_pow_20_rows(vaqlib, oracle):
    """encode_rows_locked cuts the rows in chunks of 2^20 and offsets the output by r * M codes:
    2^20 + 3 rows through the device form (the host form cuts its staging in the same chunks).  M = 2
    is no multiple of 4, which only the sequential-sum index admits; the encoder is the same kernel."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(20)
    bits, L = [4, 4], 4
    cents = gauss_cents(rng, bits, L)
    Xp = (rng.standard_normal(size=(n, 8), dtype=np.float32) * np.float32(30))
    want = oracle.encode(Xp, cents, nthreads=8)
    assert np.array_equal(want, pr.encode32(Xp, cents))
    host, dev = encode_both(plain_index(bits, cents, seq=True), Xp)
    for name, got in (("host", host), ("device", dev)):
        bad = np.nonzero((got != want).any(axis=1))[0]
        edge = {r: (got[r].tolist(), want[r].tolist()) for r in ((1 << 20) - 1, 1 << 20, (1 << 20) + 2)}
        assert bad.size == 0, f"{name} form: {bad.size} rows differ, first {bad[:5]}; rows 2^20-1, 2^20, 2^20+2: {edge}"
    sub = np.r_[0:2048, (1 << 20) - 1024:n]
    assert_encoder_guard(Xp[sub], cents, dev[sub], L)


def test_encode_u8_and_lut_chunk_loop_past_2_pow_20_rows(vaqlib):
    """The same chunk loop (one driver, encode_rows_locked, for both rules) under byte rows and under
    encodeToLUTCode's rule: 2^20 + 3 byte rows through vaqhip_encode_lut_u8[_device] and vaqhip_encode_u8[_device]
    on a sequential-sum index with D = M = 2, bits [4, 4] and the quantiles of the first 4096 rows.  Expected: the
    float calls on X.astype(float32) in two calls cut at row 600 000, so that neither reaches a chunk boundary
    (other tests tie those to the reference at small n)."""
    import torch
    n, cut = (1 << 20) + 3, 600_000
    X = np.random.default_rng(21).integers(0, 256, size=(n, 2), dtype=np.uint8)
    Xf = X.astype(np.float32)
    v = plain_index([4, 4], [], seq=True)
    v.fitQuantiles(Xf[:4096])
    d_X = torch.from_numpy(X).cuda()

    def two_calls(encode):
        parts = []
        for part in (Xf[:cut], Xf[cut:]):
            encode(part)
            parts.append(np.array(v.mCodebook))
        return np.concatenate(parts)

    def host_form(encode_u8):
        encode_u8(X)
        return np.array(v.mCodebook)

    cases = [("encode_lut_u8", two_calls(v.encodeLUT), host_form(v.encodeLUT_u8),
              v.encodeLUT_u8_device(d_X).cpu().numpy().view(np.uint16)),
             ("encode_u8", two_calls(v.encode), host_form(v.encode_u8),
              v.encode_u8_device(d_X).cpu().numpy().view(np.uint16))]
    for what, want, host, dev in cases:
        assert want.shape == (n, 2) and want.max() <= 15 and np.unique(want).size == 16
        for name, got in (("host", host), ("device", dev)):
            bad = np.nonzero((got != want).any(axis=1))[0]
            edge = {r: (got[r].tolist(), want[r].tolist()) for r in ((1 << 20) - 1, 1 << 20, (1 << 20) + 2)}
            assert bad.size == 0, (f"{what}, {name} form: {bad.size} rows differ, first {bad[:5]}; "
                                   f"rows 2^20-1, 2^20, 2^20+2: {edge}")


def test_encode_codebooks_up_to_32768_entries(vaqlib, oracle):
    """VAQHIP_MAX_BITS = 15: 32768 and 8192 centroids stream through LDS in 128 and 32 chunks of 256, next
    to a 2-entry codebook (a single short chunk)."""
    rng = np.random.default_rng(15)
    bits, L, n = [15, 1, 13, 9], 2, 300
    cents = gauss_cents(rng, bits, L)
    Xp = (rng.normal(size=(n, 8)) * 30).astype(np.float32)
    Xp[0, :L] = cents[0][32767]
    Xp[1, :L] = cents[0][256]
    want = oracle.encode(Xp, cents)
    assert np.array_equal(want, pr.encode32(Xp, cents)) and want[0, 0] == 32767 and want[1, 0] == 256
    host, dev = encode_both(plain_index(bits, cents), Xp)
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert_encoder_guard(Xp, cents, host, L)


@pytest.mark.parametrize("L", [2, 3, 5, 24, 40, 64])
def test_encode_generic_sub_vector_lengths(vaqlib, oracle, L):
    """L outside {4, 8, 16, 32}: the rows come back from an LDS tile.  launch_encode takes this
    form while 2048 * L bytes fit 160 KB of LDS, i.e. up to L = 80; 64 is the cap this test was asked to
    reach, not the kernel's limit."""
    rng = np.random.default_rng(L)
    bits, n = [6, 5, 3, 8], 700
    cents = gauss_cents(rng, bits, L)
    Xp = (rng.normal(size=(n, 4 * L)) * 30).astype(np.float32)
    want = oracle.encode(Xp, cents)
    assert np.array_equal(want, pr.encode32(Xp, cents))
    host, dev = encode_both(plain_index(bits, cents), Xp)
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert_encoder_guard(Xp, cents, host, L)


@pytest.mark.parametrize("L", [16, 5])
def test_encode_non_finite_and_extreme_rows(vaqlib, oracle, L):
    """VAQ::encodeImpl (VAQ.cpp:736-745) starts from bsf = FLT_MAX and takes a centroid on `dist < bsf`:
    a row whose distances are all NaN or infinite keeps code 0 (oracle/vaq_oracle.c, vo_encode, restates
    exactly those lines).  -0.0 equals +0.0; of two identical centroids in different 256-chunks the first
    wins."""
    bits = [9, 8, 8, 8, 8, 8, 8, 8] if L == 16 else [9, 5, 3, 8]
    Xp, cents, rows = pr.gen_encoder_planted(L, bits)
    want = oracle.encode(Xp, cents)
    host, dev = encode_both(plain_index(bits, cents), Xp)
    for got in (host, dev):
        assert got[rows["nan"], 0] == 0
        assert got[rows["inf"], 0] == 0
        assert (got[rows["huge"]] == 0).all()
        assert got[rows["negzero"], 0] == 5
        assert got[rows["dup"], 0] == 0
        assert np.array_equal(got, want)


# ====================================================================================== old refine ==
def refine_host(Xq, Xt, cand, k):
    import vaq_amd
    nq = Xq.shape[0]
    a = vaq_amd.VaqHip().refine(Xq, vaq_amd.LabelDistVec(cand.ravel(), np.zeros(cand.size, np.float32)), Xt, k)
    return a.labels.reshape(nq, k), a.distances.reshape(nq, k)


def refine_device_rc(vaqlib, Xq, Xt, cand, k):
    """vaqhip_refine_device on torch device pointers -> (rc, labels, distances)."""
    import torch
    nq, D = Xq.shape
    R = cand.shape[1]
    q, t, c = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Xq, Xt, cand))
    ol = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    od = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = vaqlib.vaqhip_refine_device(0, C.c_void_p(q.data_ptr()), nq, D, C.c_void_p(t.data_ptr()), C.c_void_p(c.data_ptr()),
                                     R, k, C.c_void_p(ol.data_ptr()), C.c_void_p(od.data_ptr()), C.c_void_p(st))
    torch.cuda.synchronize()
    return rc, ol.cpu().numpy(), od.cpu().numpy()


REFINE_GRID = [(128, R) for R in (1, 2, 3, 255, 256, 257, 2047, 2048)] + [(D, 257) for D in (1, 7, 960)]


@pytest.mark.parametrize("D,R", REFINE_GRID, ids=[f"d{d}r{r}" for d, r in REFINE_GRID])
def test_old_refine_sequential_sum_on_continuous_data(vaqlib, oracle, D, R):
    """vaqhip_refine / vaqhip_refine_device on gaussian x 30 (on integers every summation order gives the
    same bits): the sequential `acc += t * t` of include/vaqhip.h bit for bit, at R = 1, around the sort's
    power-of-two padding, at the 2048-entry cap, and k = 1, min(R, 100), R.  Host form (gathered rows)
    and device form (rows by label) are the same answer."""
    Xq, Xt, cand = pr.gen_refine_case(D, R)
    for k in sorted({1, min(R, 100), R}):
        lab, dis = pr.refine32(Xq, Xt, cand, k)
        o_lab, o_dis = oracle.refine(Xq, Xt, cand, k)
        h_lab, h_dis = refine_host(Xq, Xt, cand, k)
        rc, d_lab, d_dis = refine_device_rc(vaqlib, Xq, Xt, cand, k)
        assert rc == 0
        for name, gl, gd in (("host", h_lab, h_dis), ("device", d_lab, d_dis)):
            assert pr.same_bits(gd, dis), f"{name} D={D} R={R} k={k}: {(gd.view(np.uint32) != dis.view(np.uint32)).sum()} distances differ"
            assert np.array_equal(gl, lab), f"{name} D={D} R={R} k={k}"
            assert pr.same_bits(gd, o_dis) and np.array_equal(gl, pr.sort_tie_runs(o_lab, o_dis))
            d64 = pr.refine64_dists(Xq, Xt, gl)
            assert (np.abs(gd - d64) <= pr.sum_bound(D, d64)).all()


@pytest.mark.parametrize("k", [100, 257])
def test_old_refine_planted_cases(vaqlib, oracle, k):
    """A duplicated row (an exact tie: the smaller label first), one label twice in a list (kept twice),
    a row of 1e20 (the distance overflows) and a NaN row (neither is ever returned: the admission rule is
    dist < FLT_MAX, VAQ.cpp:867), a query whose candidates are all -1, and -1 inside and behind a list."""
    Xq, Xt, cand = pr.gen_refine_planted()
    lab, dis = pr.refine32(Xq, Xt, cand, k)
    h_lab, h_dis = refine_host(Xq, Xt, cand, k)
    rc, d_lab, d_dis = refine_device_rc(vaqlib, Xq, Xt, cand, k)
    assert rc == 0
    for name, gl, gd in (("host", h_lab, h_dis), ("device", d_lab, d_dis)):
        assert pr.same_bits(gd, dis) and np.array_equal(gl, lab), name
        assert gl[0, 0] == pr.REFINE_DUP[0] and gl[0, 1] == pr.REFINE_DUP[1]
        assert (gl[1, :2] == pr.REFINE_TWICE).all()
        assert not np.isin(gl, [pr.REFINE_HUGE, pr.REFINE_NAN]).any()
        assert (gl[pr.REFINE_EMPTY_QUERY] == -1).all() and (gd[pr.REFINE_EMPTY_QUERY] == pr.FLT_MAX).all()
        filled = gl >= 0
        d64 = pr.refine64_dists(Xq, Xt, gl)
        assert (np.abs(gd[filled] - d64[filled]) <= pr.sum_bound(Xq.shape[1], d64[filled])).all()
    for q in range(cand.shape[0]):  # the oracle on the compacted list (vo_refine reads every label it is given)
        c = cand[q][cand[q] >= 0]
        if c.size:
            o_lab, o_dis = oracle.refine(Xq[q:q + 1], Xt, c[None, :], k)
            assert pr.same_bits(h_dis[q:q + 1], o_dis) and np.array_equal(h_lab[q:q + 1], pr.sort_tie_runs(o_lab, o_dis))


def test_old_refine_refusals(vaqlib):
    import vaq_amd
    Xq, Xt, cand = pr.gen_refine_case(8, 16)
    bad = cand.copy()
    bad[2, 5] = pr.REFINE_N                      # one past the dataset: only the host form knows N
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        refine_host(Xq, Xt, bad, 4)
    assert e.value.code == EINVAL
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        refine_host(Xq, Xt, cand, 17)            # k > R
    assert e.value.code == EUNSUPPORTED
    assert refine_device_rc(vaqlib, Xq, Xt, cand, 17)[0] == EUNSUPPORTED
    Xq, Xt, cand = pr.gen_refine_case(8, 2049)
    with pytest.raises(vaq_amd._lib.VaqHipError) as e:
        refine_host(Xq, Xt, cand, 4)
    assert e.value.code == EUNSUPPORTED
    assert refine_device_rc(vaqlib, Xq, Xt, cand, 4)[0] == EUNSUPPORTED


# =========================================================================================== merge ==
def to_dev(d, l):
    import torch
    return torch.from_numpy(np.ascontiguousarray(d)).cuda(), torch.from_numpy(np.ascontiguousarray(l)).cuda()


@pytest.mark.parametrize("k", [1, 2, 127, 128, 129, 1024])
@pytest.mark.parametrize("n_lists", [1, 2, 3, 16])
def test_merge_fold_counts_and_fill_levels(vaqlib, n_lists, k):
    """merge_kernel folds through a 2048-entry buffer: 16 lists of k = 128 are exactly one sort, k = 129 the
    first shape that folds twice, k = 1024 folds once per list.  Lists are empty, hold one entry, half,
    all but one or all of their k slots; one query has nothing at all; in one the k-th and (k+1)-th
    entries tie in different lists and the smaller label must win.  Dense, packed and strided forms."""
    import torch
    from vaq_amd.index import merge_topk_device, merge_topk_packed_device
    d, l = pr.gen_merge_case(n_lists, k)
    nq = pr.MERGE_NQ
    want_l, want_d = pr.merge_ref(d, l, k)
    td, tl = to_dev(d, l)
    out_l, out_d = merge_topk_device(td, tl, k)
    torch.cuda.synchronize()
    got_l, got_d = out_l.cpu().numpy(), out_d.cpu().numpy()
    assert pr.same_bits(got_d, want_d), f"rows {np.nonzero((got_d != want_d).any(axis=1))[0]}"
    assert np.array_equal(got_l, want_l), f"rows {np.nonzero((got_l != want_l).any(axis=1))[0]}"
    # [world, 2, nq, k]: plane 0 labels, plane 1 distance bits
    packed = torch.stack([tl, td.view(torch.int32)], dim=1).contiguous()
    out_l, out_d = merge_topk_packed_device(packed, n_lists, nq, k)
    torch.cuda.synchronize()
    assert np.array_equal(out_l.cpu().numpy(), want_l) and pr.same_bits(out_d.cpu().numpy(), want_d)
    # padded strides, the padding poisoned with (distance 0, label 0): no real label is 0
    qs, pad = k + 5, 13
    ls = nq * qs + pad
    sd = np.zeros((n_lists, ls), np.float32)
    sl = np.zeros((n_lists, ls), np.int32)
    for i in range(n_lists):
        for q in range(nq):
            sd[i, q * qs:q * qs + k] = d[i, q]
            sl[i, q * qs:q * qs + k] = l[i, q]
    tsd, tsl = to_dev(sd, sl)
    out_l = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    out_d = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = vaqlib.vaqhip_merge_topk_strided_device(0, C.c_void_p(tsd.data_ptr()), C.c_void_p(tsl.data_ptr()), n_lists, ls, qs, nq, k,
                                                 C.c_void_p(out_l.data_ptr()), C.c_void_p(out_d.data_ptr()), C.c_void_p(st))
    torch.cuda.synchronize()
    assert rc == 0
    got_l, got_d = out_l.cpu().numpy(), out_d.cpu().numpy()
    assert not (got_l == 0).any()
    assert np.array_equal(got_l, want_l) and pr.same_bits(got_d, want_d)


def test_merge_packed_world_3_and_large_labels(vaqlib):
    """Labels up to 2^31 - 2 (the largest vaqhip_index_set_codes_u16 admits with id_base) merge like any other."""
    import torch
    from vaq_amd.index import merge_topk_device, merge_topk_packed_device
    k, world = 128, 3
    d, l = pr.gen_merge_case(world, k, label_top=2 ** 31 - 2)
    want_l, want_d = pr.merge_ref(d, l, k)
    assert want_l.max() >= 2 ** 31 - 2 - 4 * l.size
    td, tl = to_dev(d, l)
    for out_l, out_d in (merge_topk_device(td, tl, k),
                         merge_topk_packed_device(torch.stack([tl, td.view(torch.int32)], dim=1).contiguous(), world, pr.MERGE_NQ, k)):
        torch.cuda.synchronize()
        assert np.array_equal(out_l.cpu().numpy(), want_l) and pr.same_bits(out_d.cpu().numpy(), want_d)


def test_merge_limits(vaqlib):
    import torch
    nq, k = 4, 9
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_l = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    out_d = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    po = (C.c_void_p(out_l.data_ptr()), C.c_void_p(out_d.data_ptr()))
    # no lists: every slot -1 / FLT_MAX
    assert vaqlib.vaqhip_merge_topk_device(0, None, None, 0, nq, k, *po, st) == 0
    torch.cuda.synchronize()
    assert (out_l.cpu().numpy() == -1).all() and (out_d.cpu().numpy() == pr.FLT_MAX).all()
    # no queries: succeeds and writes nothing
    out_l.fill_(-7)
    out_d.fill_(-7.0)
    d, l = to_dev(np.zeros((2, 1, k), np.float32), np.ones((2, 1, k), np.int32))
    pi = (C.c_void_p(d.data_ptr()), C.c_void_p(l.data_ptr()))
    assert vaqlib.vaqhip_merge_topk_device(0, *pi, 2, 0, k, *po, st) == 0
    torch.cuda.synchronize()
    assert (out_l.cpu().numpy() == -7).all() and (out_d.cpu().numpy() == -7.0).all()
    # more than 16 lists, k above VAQHIP_MAX_K: refused before anything is read
    assert vaqlib.vaqhip_merge_topk_device(0, *pi, 17, nq, k, *po, st) == EUNSUPPORTED
    assert vaqlib.vaqhip_merge_topk_device(0, *pi, 2, nq, 1025, *po, st) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (out_l.cpu().numpy() == -7).all()


# ================================================================== merge levels above 16 lists ==
_slice_cache = {}


def slice_case(oracle):
    if not _slice_cache:
        from helpers import make_case
        c = make_case(4040, 128, [8] * 8, 40000, 3, dup_frac=0.02)
        Xp = oracle.project(c["X"], c["eig"])
        luts = [oracle.create_lut(Xp[q], c["cents"], 8) for q in range(3)]
        _slice_cache.update(c=c, Xp=Xp, ad=np.stack([oracle.all_dists(t, c["codes"]) for t in luts]))
    return _slice_cache["c"], _slice_cache["Xp"], _slice_cache["ad"]


@pytest.mark.parametrize("k", [1, 100, 1000])
def test_merge_levels_above_16_lists_through_a_search(vaqlib, oracle, k):
    """More than 16 partial lists per query are reachable only through a search with many row slices.
    launch_merge then has two first levels, and which one runs is the search's choice:

      * without per-list counts, the 16-way fan-in loop: merge_kernel(final = 0) over groups of 16 lists,
        then the final merge_kernel -- the plain multi-slice scan ("ordered_slices" 0; at this size the
        seeding pre-pass, the other source of counts, needs 256 slices and 2^21 rows and stays off);
      * with the scan's per-list counts, merge_compact_kernel (count scan, gather of up to 256 lists, its
        own fold) -- option "ordered_slices" 1, which makes the scan publish its counts for any 1 < slices
        <= 4096.

    N = 40 000 rows of 8-byte codes; the plan rounds a slice up to one step of the largest workgroup (2048
    rows), so it grants ceil(40000 / 2048) = 20 slices at most -- asking for 255, 256 or 257 gives 20,
    asking for 16 or 17 gives 10.  More than 256 lists (a second compacting group, two fan-in levels) would
    need more than 256 * 2048 rows and stay with the 1M-row tests of tests/test_parity_gpu.py.  The
    interface reports neither the merge level nor `ordered`; what it does report is asserted: the slice
    count actually used, and -- at 4 slices, where the best-first form runs -- that the option displaces
    that form, which the plan never combines with the slice order."""
    c, Xp, ad = slice_case(oracle)
    v = plain_index(c["bits"], c["cents"], eig=c["eig"], codes=c["codes"])
    o_lab, o_dis = oracle.search(Xp, c["cents"], c["codes"], k, max_bits=8, projected=True)
    used = {}
    for order in (0, 1):
        for bf in (0, 1):
            for slices in (16, 17, 255, 256, 257):
                v.set_option("ordered_slices", order)
                v.set_option("best_first", bf)
                v.set_option("slices", slices)
                v.set_option("timing", 1)
                a = v.search(c["X"], k)
                t = v.last_timing()
                used[(order, bf, slices)] = t["slices"]
                v.set_option("timing", 0)
                assert_topk_matches(a.labels.reshape(3, k), a.distances.reshape(3, k), o_lab, o_dis, ad,
                                    what=f"k={k} ordered_slices={order} best_first={bf} slices={slices} (ran {t['slices']})")
    for order in (0, 1):  # fan-in loop (0) and compacting level (1): each above and below 16 lists
        got = [used[(order, bf, s)] for bf in (0, 1) for s in (16, 17, 255, 256, 257)]
        assert max(got) > 16 and min(got) <= 16, used
        assert max(got) == -(-40000 // 2048), used            # the plan's clamp, as the docstring says
    # The slice order was honoured on this index: at 4 slices the best-first form runs without it and is
    # displaced by it (the plan never combines the two).  The other terms of the plan's condition -- the
    # bucket count, the bucket key, 1 < slices <= 4096 -- are the same at 20 slices.
    probe = {}
    for order in (0, 1):
        v.set_option("ordered_slices", order)
        v.set_option("best_first", 1)
        v.set_option("slices", 4)
        v.set_option("timing", 1)
        a = v.search(c["X"], k)
        t = v.last_timing()
        v.set_option("timing", 0)
        probe[order] = (t["slices"], t["best_first"])
        assert_topk_matches(a.labels.reshape(3, k), a.distances.reshape(3, k), o_lab, o_dis, ad, what=f"k={k} probe order={order}")
    assert probe == {0: (4, 1), 1: (4, 0)}, probe
