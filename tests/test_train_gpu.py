"""Training from raw rows on the device: the second moment in its documented order, the Jacobi solver against its
host twin, the composite against the decisions recorded from the reference (tests/golden/train), and the chain into an
index.  Shapes: the smallest that reach every path (one ragged tile, two tiles, the sampled branch, many blocks)."""
import ctypes as C

import numpy as np
import pytest

import train_ref as tr

pytestmark = pytest.mark.gpu
EINVAL = -1
p = tr._p


def _rows(seed, n, D):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal((n, D)) * rng.uniform(0.1, 30.0, D)).astype(np.float32)


def _moment_host(vaqlib, X):
    n, D = X.shape
    cov, cov_f = np.full((D, D), -7.0), np.full((D, D), -7.0, np.float32)
    fn = vaqlib.vaqhip_train_moment_u8 if X.dtype == np.uint8 else vaqlib.vaqhip_train_moment
    assert fn(0, p(X), n, D, p(cov), p(cov_f)) == 0, vaqlib.vaqhip_last_error()
    return cov, cov_f


def _moment_device(vaqlib, X, odd=False):
    import torch
    n, D = X.shape
    if odd:  # byte rows at an odd address
        buf = torch.zeros(n * D + 3, dtype=torch.uint8, device="cuda")
        d_X = buf[3:3 + n * D].view(n, D)
        d_X.copy_(torch.from_numpy(X))
    else:
        d_X = torch.from_numpy(X).cuda()
    d_cov = torch.full((D, D), -7.0, dtype=torch.float64, device="cuda")
    d_cov_f = torch.full((D, D), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fn = vaqlib.vaqhip_train_moment_u8_device if X.dtype == np.uint8 else vaqlib.vaqhip_train_moment_device
    assert fn(0, C.c_void_p(d_X.data_ptr()), n, D, C.c_void_p(d_cov.data_ptr()), C.c_void_p(d_cov_f.data_ptr()), None) == 0
    return d_cov.cpu().numpy(), d_cov_f.cpu().numpy()


def _moment_refiner(X):
    import vaq_amd
    r = vaq_amd.VaqRefiner(X.shape[1])
    (r.set_rows_u8 if X.dtype == np.uint8 else r.set_rows)(X)
    out = r.train_moment()
    r.close()
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


MOMENT_SHAPES = [(7, 5), (1025, 33), (2001, 2), (1001, 1), (3000, 128)]


@pytest.fixture(scope="module")
def moment_refs():
    return {s: (lambda X: (X, tr.moment_ref(X)))(_rows(100 + i, *s)) for i, s in enumerate(MOMENT_SHAPES)}


@pytest.mark.parametrize("shape", MOMENT_SHAPES)
def test_moment_equals_its_documented_order(vaqlib, moment_refs, shape):
    X, want = moment_refs[shape]
    cov, cov_f = _moment_host(vaqlib, X)
    assert _same_bits(cov, want), np.max(np.abs(cov - want))
    assert _same_bits(cov, cov.T)
    assert _same_bits(cov_f, want.astype(np.float32))
    for what, (c, cf) in (("_device", _moment_device(vaqlib, X)), ("refiner", _moment_refiner(X))):
        assert _same_bits(c, cov) and _same_bits(cf, cov_f), what


@pytest.mark.parametrize("name", [c for c in sorted(tr.CASES) if c != "bytes"])
def test_moment_within_gamma_of_the_reference(vaqlib, name):
    """|ours - covmat| <= gamma_n sum_r |x_ri x_rj| entry by entry: the standard bound of the reference's float GEMM
    against the exact sum, which our double sum equals up to 2^-29 of that bound's scale.  gamma_n as derived, not widened."""
    X = tr.make_inputs(name)
    fx = tr.load_fixture(name)
    cov, _ = _moment_host(vaqlib, X)
    assert _same_bits(cov, tr.moment_ref(X))
    rows = len(tr.sample_rows(*X.shape))
    bound = tr.gamma(rows) * tr.moment_abs(X)
    err = np.abs(cov - fx["covmat"].astype(np.float64))
    print(f"{name}: max |ours - covmat| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("which", ["fixture", "wide"])
def test_moment_bytes_is_the_exact_integer(vaqlib, which):
    if which == "fixture":
        X = tr.make_inputs("bytes")
    else:
        X = np.random.Generator(np.random.PCG64(9)).integers(0, 256, (5000, 128), dtype=np.uint8)
    S = X[tr.sample_rows(*X.shape)].astype(np.int64)
    want = (S.T @ S).astype(np.float64)
    assert np.max(want) < 2.0 ** 53
    cov, cov_f = _moment_host(vaqlib, X)
    assert _same_bits(cov, want)
    widened, widened_f = _moment_host(vaqlib, X.astype(np.float32))
    assert _same_bits(widened, cov) and _same_bits(widened_f, cov_f)
    for what, (c, cf) in (("_u8_device", _moment_device(vaqlib, X)), ("_u8_device odd", _moment_device(vaqlib, X, odd=True)),
                          ("refiner", _moment_refiner(X))):
        assert _same_bits(c, cov) and _same_bits(cf, cov_f), what
    if which == "fixture":
        fx = tr.load_fixture("bytes")
        assert np.all(np.abs(cov - fx["covmat"].astype(np.float64)) <= tr.gamma(X.shape[0]) * want)


def test_moment_nan_row_propagates(vaqlib):
    X = _rows(3, 50, 8)
    X[17, 2] = np.nan
    cov, _ = _moment_host(vaqlib, X)
    assert np.isnan(cov[2]).all() and np.isnan(cov[:, 2]).all()
    assert np.isfinite(np.delete(np.delete(cov, 2, 0), 2, 1)).all()
    eig, bits, hi = np.zeros((8, 8), np.float32), np.zeros(4, np.int32), C.c_int(0)
    assert vaqlib.vaqhip_train_rotation(0, p(X), 50, 8, 4, 16, 1, 8, 1.0, p(eig), None, p(bits), C.byref(hi)) == EINVAL
    assert b"NaN" in vaqlib.vaqhip_last_error()


# ---- the solver ----
def _eigen_device(vaqlib, A):
    import torch
    D = A.shape[0]
    d_A = torch.from_numpy(np.array(A, np.float64, order="C")).cuda()
    d_val = torch.zeros(D, dtype=torch.float64, device="cuda")
    d_vec = torch.zeros((D, D), dtype=torch.float64, device="cuda")
    sweeps = C.c_int(-1)
    torch.cuda.synchronize()
    rc = vaqlib.vaqhip_sym_eigen_device(0, C.c_void_p(d_A.data_ptr()), D, C.c_void_p(d_val.data_ptr()),
                                        C.c_void_p(d_vec.data_ptr()), C.byref(sweeps), None)
    return rc, d_val.cpu().numpy(), d_vec.cpu().numpy(), sweeps.value


@pytest.mark.parametrize("name", ["d1", "d2", "d3", "d5", "d64", "diagonal", "repeated", "zero", "graded", "d129"])
def test_device_jacobi_equals_the_host(vaqlib, name):
    if name == "d129":
        B = np.random.Generator(np.random.PCG64(129)).standard_normal((129, 129))
        A = (B + B.T) / 2
    else:
        A = tr.eigen_matrices()[name]
    rc, values, vectors, sweeps = _eigen_device(vaqlib, A)
    h_rc, h_values, h_vectors, h_sweeps = tr.sym_eigen_host(vaqlib, A)
    assert rc == 0 and h_rc == 0
    assert 0 <= sweeps <= tr.MAX_SWEEPS and sweeps == h_sweeps
    if name in ("diagonal", "zero", "d1"):
        assert sweeps == 0
    assert _same_bits(values, h_values), np.max(np.abs(values - h_values))
    assert _same_bits(vectors, h_vectors), np.max(np.abs(vectors - h_vectors))


def test_device_jacobi_refuses_non_finite(vaqlib):
    A = np.eye(5)
    A[3, 1] = np.inf
    rc, _, _, sweeps = _eigen_device(vaqlib, A)
    assert rc == EINVAL and sweeps == 0


# ---- the composite ----
def _expected_bits(vaqlib, fx, last_lb):
    """The exact solver on the recorded coefficients.  At percent_var = 1 the last lower bound hangs on a float sum that
    is 1 up to an ulp (tests/test_train_cpu.py names the fixtures where it moves the bits): that one bound is `last_lb`,
    the plan's from the device's own eigenvalues."""
    H = int(fx["highest_subs"])
    lb = np.where(fx["cum_var"][:H] <= np.float32(fx["percent_var"]), int(fx["min_bits"]), 0)
    if float(fx["percent_var"]) >= 1:
        lb[-1] = last_lb
    got = tr.allocate_bits(vaqlib, fx["var_per_subs"][:H], lb, int(fx["max_bits"]), fx["k"], int(fx["bit_budget"]))
    assert not isinstance(got, int), got
    return got[0]


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_composite_takes_the_references_decisions(vaqlib, name):
    """Orders, surviving swaps, highest_subs, k and the bits equal what the reference decided from ITS eigenvalues; the
    eigenvectors are compared through what they must do (diagonalise XtX in the balanced order)."""
    import vaq_amd
    X = tr.make_inputs(name)
    fx = tr.load_fixture(name)
    n, D, M = (int(v) for v in fx["shape"])
    args = (M, int(fx["bit_budget"]), int(fx["min_bits"]), int(fx["max_bits"]), float(fx["percent_var"]))
    eig, ev, bits, hi = vaq_amd.train_rotation(X, *args)
    t = vaq_amd.last_train_timing()
    assert t["sample_rows"] == len(tr.sample_rows(n, D)) and t["rows"] == n and 0 <= t["sweeps"] <= tr.MAX_SWEEPS
    assert hi == int(fx["highest_subs"])
    ref_ev = fx["eigenvalues"][fx["balanced"]]
    if name == "deficient":
        # only what the 5 non-zero eigenvalues decide (README): the leading values, the first k, highest_subs
        lead = np.argsort(-ev)[:5]
        assert np.allclose(np.sort(ev)[::-1][:5], np.sort(fx["eigenvalues"])[::-1][:5], rtol=1e-4)
        assert np.array_equal(np.sort(lead), np.sort(np.argsort(-ref_ev)[:5]))
        assert len(bits) == hi and sum(bits) == int(fx["bit_budget"])
        ours = tr.train_plan(vaqlib, np.sort(ev)[::-1].copy(), M, args[4], args[2], args[3])
        assert ours["swaps_kept"] == int(fx["swaps_kept"]) and ours["highest"] == hi
        assert np.array_equal(ours["k"][:1], fx["k"][:1])
        assert np.allclose(ours["var"][:2], fx["var_per_subs"][:2], rtol=1e-5)
    else:
        # the same columns moved: our values, in the order returned, rank as the reference's balanced ones do
        assert np.array_equal(np.argsort(-ev, kind="stable"), np.argsort(-ref_ev, kind="stable"))
        ours = tr.train_plan(vaqlib, np.sort(ev)[::-1].copy(), M, args[4], args[2], args[3])
        assert ours["swaps_kept"] == int(fx["swaps_kept"]) and ours["highest"] == hi
        assert np.array_equal(ours["k"], fx["k"])
        assert bits == _expected_bits(vaqlib, fx, int(ours["lb"][-1]))
    # the rotation: orthonormal, and it diagonalises the second moment with the returned values on the diagonal
    cov = tr.moment_ref(X)
    E = eig.astype(np.float64)
    scale = float(np.max(np.abs(np.linalg.eigvalsh(cov))))
    assert np.max(np.abs(E.T @ E - np.eye(D))) < 16 * D * 2.0 ** -24
    assert np.max(np.abs(E.T @ cov @ E - np.diag(ev.astype(np.float64)))) < 16 * D * 2.0 ** -24 * scale
    big = np.argmax(np.abs(eig), axis=0)
    assert np.all(eig[big, np.arange(D)] > 0)
    # every form gives the same bits
    r = vaq_amd.VaqRefiner(D)
    (r.set_rows_u8 if X.dtype == np.uint8 else r.set_rows)(X)
    r_eig, r_ev, r_bits, r_hi = r.train_rotation(*args)
    r.close()
    assert _same_bits(r_eig, eig) and _same_bits(r_ev, ev) and r_bits == bits and r_hi == hi
    import torch
    d_eig, d_ev, d_bits, d_hi = vaq_amd.train_rotation(torch.from_numpy(X).cuda(), *args)
    assert _same_bits(d_eig, eig) and _same_bits(d_ev, ev) and d_bits == bits and d_hi == hi
    if X.dtype == np.uint8:
        w_eig, w_ev, w_bits, w_hi = vaq_amd.train_rotation(X.astype(np.float32), *args)
        assert _same_bits(w_eig, eig) and _same_bits(w_ev, ev) and w_bits == bits and w_hi == hi


def test_chained_forms_refuse_what_cannot_be_fitted():
    import vaq_amd
    X = tr.make_inputs("percent")
    with pytest.raises(vaq_amd.VaqHipError) as e:
        vaq_amd.train(X, 4, 8, 1, 8, percent_var=0.9)
    assert e.value.code == -2


# ---- end to end ----
def _blobs(n, D, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.standard_normal((12, D)) * rng.uniform(1.0, 12.0, D)
    return (centres[rng.integers(0, 12, n)] + rng.standard_normal((n, D))).astype(np.float32)


@pytest.mark.parametrize("resident", [False, True])
def test_train_to_search(vaqlib, resident):
    """train -> index -> encode -> search; the index rebuilt through the existing calls with the returned eigvec and
    bits passed by hand answers the same: the new outputs are in the shape the rest of the library takes."""
    import vaq_amd
    X = _blobs(3000, 16, 41)
    Q = _blobs(32, 16, 42)
    if resident:
        r = vaq_amd.VaqRefiner(16)
        r.set_rows(X)
        eig, bits, cents = r.train(4, 16, 1, 8)
        r.close()
    else:
        eig, bits, cents = vaq_amd.train(X, 4, 16, 1, 8)
    assert len(bits) == 4 and sum(bits) == 16 and all(1 <= b <= 8 for b in bits)
    assert [c.shape for c in cents] == [(1 << b, 4) for b in bits]

    def answers(eigvec, bits_, centres):
        v = vaq_amd.VaqHip()
        v.mBitsAlloc = list(bits_)
        v.mCentroidsPerSubs = centres
        v.mEigenVectors = eigvec
        v.encode(X, projected=False)
        out = v.search(Q, 10)
        return np.asarray(out.labels).copy(), np.asarray(out.distances).copy()

    labels, dists = answers(eig, bits, cents)
    by_hand, _, _ = vaq_amd.fit_codebooks(X, 4, [int(b) for b in bits], eigvec=eig.copy())
    h_labels, h_dists = answers(eig.copy(), [int(b) for b in bits], by_hand)
    assert np.array_equal(labels, h_labels) and _same_bits(dists, h_dists)
    assert labels.min() >= 0 and labels.max() < 3000
    # the variance-aware allocation hands the leading subspace at least as many bits as the last
    assert bits[0] >= bits[-1]


@pytest.mark.parametrize("extra", [[], ["--refine-resident"], ["--file-format-ori", "bvecs"]], ids=["fvecs", "resident", "bvecs"])
def test_demo_trains_encodes_and_searches(vaqlib, tmp_path, extra):
    """demo_vaqhip --train --bit-budget B --subspaces M --dataset ... --encode: from a file of raw rows to answers with no
    foreign input (the C++ adapter's train / trainRefineDataset); the bits it prints, the codes it saves and the
    labels it writes equal the Python chain's on the same rows."""
    import subprocess
    import vaq_amd
    from vaq_amd import build, io
    exe = build.build_demo()
    bvecs = "bvecs" in extra
    X = _blobs(3000, 16, 41)
    Q = _blobs(9, 16, 43)
    if bvecs:
        X = np.clip(np.rint(X * 4 + 128), 0, 255).astype(np.uint8)
        Q = np.clip(np.rint(Q * 4 + 128), 0, 255).astype(np.uint8)
    io.write_vecs(str(tmp_path / ("base.bvecs" if bvecs else "base.fvecs")), X)
    io.write_vecs(str(tmp_path / ("q.bvecs" if bvecs else "q.fvecs")), Q)
    k = 5
    r = subprocess.run([exe, "--train", "--bit-budget", "16", "--subspaces", "4", "--min-bits", "1", "--max-bits", "8",
                        "--dataset", str(tmp_path / ("base.bvecs" if bvecs else "base.fvecs")), "--encode",
                        "--timeseries-size", "16", "--queries", str(tmp_path / ("q.bvecs" if bvecs else "q.fvecs")),
                        "--k", str(k), "--save-enc", str(tmp_path / "cb.bin"), "--result", str(tmp_path / "out.csv")] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    eig, bits, cents = vaq_amd.train(X, 4, 16, 1, 8)
    assert "bit allocation: " + "".join(f"{b}, " for b in bits) in r.stdout and "Jacobi sweeps" in r.stdout
    v = vaq_amd.VaqHip()
    v.mBitsAlloc, v.mCentroidsPerSubs, v.mEigenVectors = list(bits), cents, eig
    Xf, Qf = X.astype(np.float32), Q.astype(np.float32)
    v.encode(Xf, projected=False)
    assert np.array_equal(io.load_codebook(str(tmp_path / "cb.bin")), v.mCodebook)
    labels = np.asarray(v.search(Qf, k).labels).reshape(-1, k)
    v.close()
    assert np.array_equal(np.loadtxt(str(tmp_path / "out.csv"), delimiter=",", dtype=np.int64), labels.astype(np.int64))
