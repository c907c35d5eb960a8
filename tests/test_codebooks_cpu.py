"""The subspace codebook fit on the CPU: tests/codebooks_ref.py (per subspace tests/kmeans_ref.py's restatement of
KMeans::staticFitSampling on the rows that call takes: all of them in order, or its prefix of the sample) against
the fixtures recorded from the reference itself (tests/golden/codebooks/README.md); the symbols; every refusal made before a device is touched; and the host arithmetic
of vaq_amd/csrc/fit_codebooks_plan.h through its stand-alone program (tests/cpp/fit_codebooks_plan_test.cpp, once more
under AddressSanitizer + UBSan: host code only, its own main)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import codebooks_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(cr.CASES)
NEW_SYMBOLS = ("vaqhip_fit_codebooks", "vaqhip_fit_codebooks_device", "vaqhip_fit_codebooks_u8",
               "vaqhip_fit_codebooks_u8_device", "vaqhip_refiner_fit_codebooks", "vaqhip_fit_codebooks_set_timing",
               "vaqhip_last_fit_codebooks_timing")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ---- digests first --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_inputs_are_the_recorded_ones(name):
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = cr.make_inputs(name)
    fx = cr.load_fixture(name)
    assert X.shape == (n, D) and X.dtype == (np.uint8 if kind in ("bytes", "bits01") else np.float32)
    assert (eig is not None) == (kind == "rotated")
    assert tuple(int(v) for v in fx["shape"]) == (n, D, M) and tuple(int(b) for b in fx["bits"]) == bits
    assert int(fx["max_iter"]) == cr.MAX_ITER
    assert str(fx["inputs_digest"]) == cr.digest(X, eig), "numpy no longer generates the recorded inputs"


@pytest.fixture(scope="module")
def fits():
    """Every case fitted once by the restatement, shared by the tests below."""
    out = {}
    for name in CASES:
        n, D, M, bits, kind, salt = cr.CASES[name]
        X, eig = cr.make_inputs(name)
        out[name] = cr.fit_codebooks(X, M, bits, eig)
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(fits, name):
    n, D, M, bits, kind, salt = cr.CASES[name]
    fx = cr.load_fixture(name)
    cents, iters, nans = fits[name]
    for s in range(M):
        cr.assert_centres_equal(cents[s], fx["centres_%d" % s], f"{name}, subspace {s}")
        assert iters[s] == int(fx["iterations_%d" % s])
        assert np.array_equal(nans[s], fx["nan_rows_%d" % s])
        assert np.array_equal(np.isnan(fx["centres_%d" % s]).any(axis=1), fx["nan_rows_%d" % s])


def test_every_case_shows_what_it_names():
    """The table of the README: no run under three iterations; NaN centres run to the cap; the sampled cases show a
    NaN subspace beside one without, `prefix` and `bytes` also a subspace that converges early beside one at the cap;
    `mixed` and the launch-shape cases the conditions their rows name."""
    fx = {n: cr.load_fixture(n) for n in CASES}
    its = {n: [int(fx[n]["iterations_%d" % s]) for s in range(cr.CASES[n][2])] for n in CASES}
    nan = {n: [int(fx[n]["nan_rows_%d" % s].sum()) for s in range(cr.CASES[n][2])] for n in CASES}
    for n in CASES:
        assert min(its[n]) >= 3, n
        for s, c in enumerate(nan[n]):  # a NaN centre never compares equal: the loop cannot stop early
            assert c == 0 or its[n][s] == cr.MAX_ITER, (n, s)
    assert all(i < cr.MAX_ITER for i in its["tiny"]) and len(set(cr.CASES["tiny"][3])) == 4
    assert cr.CASES["odd"][0] % 2 == 1 and cr.CASES["odd"][1] // cr.CASES["odd"][2] == 12  # halves differ; a packet and a tail
    for n in ("sampled", "prefix"):
        assert cr.CASES[n][0] > cr.MIN_SAMPLE and max(nan[n]) > 0 and min(nan[n]) == 0, n
    assert [cr.sample_count(140000, 1 << b) for b in cr.CASES["prefix"][3]] == [131072, 65536]
    for n in ("prefix", "bytes"):
        assert max(its[n]) == cr.MAX_ITER and min(its[n]) < cr.MAX_ITER, n
    assert min(nan["bytes"][:2]) > 0 and nan["bytes"][3] == 0
    assert len(np.unique(cr.make_inputs("bytes")[0][:, :2], axis=0)) <= 16 < 32
    assert sum(nan["rotated"]) == 0 and cr.CASES["rotated"][2] % 4 == 0
    assert cr.CASES["wide"][1] * 4 * 64 > 40 * 1024  # a 64-row tile of such slices does not fit the LDS tile
    # mixed: the sampling decision is each subspace's own, a sampling one before and after the one that does not
    n, D, M, bits, kind, salt = cr.CASES["mixed"]
    assert [cr.sampled(n, 1 << b) for b in bits] == [True, False, True]
    assert [cr.sample_count(n, 1 << b) for b in bits] == [65536, 66000, 65536]
    _launch_shape_cases()


def _slices(name):
    """(L, [per subspace the dense rows the reference's call works on]) of an unsampled case"""
    n, D, M, bits, kind, salt = cr.CASES[name]
    assert not any(cr.sampled(n, 1 << b) for b in bits)
    P = cr.projected_rows(*cr.make_inputs(name))
    return D // M, [cr.subspace_rows(P, n, D, M, bits, s) for s in range(M)]


def _launch_shape_cases():
    """The launch-shape rows of the README's table, from the rules of codebooks_fit restated in cr.assign_launch."""
    # staged: two turns of the centre staging loop, the second clipped; rows on both sides of the boundary
    n, D, M, bits, kind, salt = cr.CASES["staged"]
    L, rows = _slices("staged")
    k = 1 << bits[0]
    R, x_lds, stage = cr.assign_launch(L, max(1 << b for b in bits))
    assert (L, R, x_lds, stage) == (12, 256, True, 341) and cr.STAGE_FLOATS // L < k and k % (cr.STAGE_FLOATS // L) != 0
    assert [min(stage, k - c0) for c0 in range(0, k, stage)] == [341, 171]
    assert (1 << bits[1]) < stage  # the second subspace's only turn is clipped by its k
    last = cr.assign(rows[0], cr.load_fixture("staged")["centres_0"])
    assert (last < stage).any() and (last >= stage).any() and (last >= 0).all()
    # dupes: an identical seed on either side of the stage boundary, a row at distance 0 from both
    n, D, M, bits, kind, salt = cr.CASES["dupes"]
    L, rows = _slices("dupes")
    k = 1 << bits[0]
    R, x_lds, stage = cr.assign_launch(L, k)
    assert (stage, k) == (512, 1024) and len(np.unique(rows[0], axis=0)) <= 256
    heads = cr.permutation_head(n, k)
    seeds = rows[0][heads]
    first = {}
    for i in range(stage):
        first.setdefault(seeds[i].tobytes(), i)
    pairs = [(first[seeds[j].tobytes()], j) for j in range(stage, k) if seeds[j].tobytes() in first]
    assert pairs
    i, j = pairs[0]
    assert i < stage <= j and np.array_equal(seeds[i], seeds[j]) and np.array_equal(rows[0][heads[i]], seeds[j])
    fx = cr.load_fixture("dupes")
    assert int(fx["iterations_0"]) == cr.MAX_ITER and int(fx["nan_rows_0"].sum()) == 773
    # the tiers of the row tile, both sides of every boundary; a row stride that is not the slice length
    got = []
    for name, L in cr.TIERS.items():
        n, D, M, bits, kind, salt = cr.CASES[name]
        assert D // M == L and M == 2 and D != L
        R, x_lds, stage = cr.assign_launch(L, max(1 << b for b in bits))
        assert n % R != 0 and n > R  # ragged, more than one workgroup
        got.append(R if x_lds else "global")
    assert got == [256, 128, 128, 64, 64, "global"]
    # wide_staged: the global path in two turns
    n, D, M, bits, kind, salt = cr.CASES["wide_staged"]
    R, x_lds, stage = cr.assign_launch(D // M, 1 << bits[0])
    assert (R, x_lds, stage) == (64, False, 25) and (1 << bits[0]) * D > cr.STAGE_FLOATS and (1 << bits[0]) % stage == 7
    # the odd lengths: one column; three packets (the third joins after the accumulators) and a tail of 3
    assert cr.CASES["len1"][1] // cr.CASES["len1"][2] == 1
    L = cr.CASES["len27"][1] // cr.CASES["len27"][2]
    assert (L // 8, L % 8, (L // 16) * 16) == (3, 3, 16)


def test_lloyd_lowers_the_cost_on_rotated(fits):
    """What the GPU end-to-end test asserts of the fitted index, checked here on the recorded centres: strictly lower
    mean squared distance to the nearest centre than with the seed centres, in every subspace."""
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = cr.make_inputs("rotated")
    P = cr.projected_sample(X, eig, bits).astype(np.float64)
    L = D // M
    for s in range(M):
        Ps = P[:, s * L:(s + 1) * L]

        def cost(c):
            return ((Ps[:, None, :] - c[None, :, :]) ** 2).sum(-1).min(1).mean()
        assert cost(fits["rotated"][0][s].astype(np.float64)) < cost(Ps[cr.permutation_head(n, 1 << bits[s])]), s


# ---- the library without a device --------------------------------------------------------------------------------
def test_symbols_version_and_python_names(vaqlib):
    import vaq_amd
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 120
    for name in NEW_SYMBOLS:
        assert hasattr(vaqlib, name) and name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "vaqhip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    for name in ("fit_codebooks", "fit_codebooks_u8", "fit_codebooks_timing", "last_fit_codebooks_timing"):
        assert callable(getattr(vaq_amd, name)) and name in vaq_amd.__all__
    assert callable(vaq_amd.VaqRefiner.fit_codebooks)
    assert C.sizeof(_lib.FitCodebooksTiming()) == 5 * 4 + 3 * 4 + 2 * 8


def _call(fn, X, n, D, M, bits, max_iter=25, cent="out", device_form=False):
    out = np.full(1 << 12, 7.25, np.float32)
    iters = np.full(max(M, 1), -9, np.int32)
    nan = np.full(max(M, 1), -9, np.int32)
    b = (C.c_int * max(len(bits), 1))(*bits) if bits is not None else None
    args = [0, _p(X), n, D, M, b, None, max_iter, _p(out) if cent == "out" else None, _p(iters), _p(nan)]
    rc = fn(*(args + [None] if device_form else args))
    assert np.all(out == 7.25) and np.all(iters == -9) and np.all(nan == -9), "a refusal wrote to an output"
    return rc


def test_refused_before_a_device_is_touched(vaqlib):
    """Every refusal of the header, in the four forms; each _u8 form with its float twin's code; the outputs untouched."""
    Xf, X8 = np.zeros((300, 8), np.float32), np.zeros((300, 8), np.uint8)
    forms = [(vaqlib.vaqhip_fit_codebooks, Xf, False), (vaqlib.vaqhip_fit_codebooks_u8, X8, False),
             (vaqlib.vaqhip_fit_codebooks_device, Xf, True), (vaqlib.vaqhip_fit_codebooks_u8_device, X8, True)]
    EINVAL, EUNSUPPORTED = -1, -2
    big_m = 129
    cases = [
        ("null X", dict(X=None, n=300, D=8, M=4, bits=[2] * 4), EINVAL),
        ("null bits", dict(n=300, D=8, M=4, bits=None), EINVAL),
        ("null centroids", dict(n=300, D=8, M=4, bits=[2] * 4, cent=None), EINVAL),
        ("n < 1", dict(n=0, D=8, M=4, bits=[2] * 4), EINVAL),
        ("n >= 2^31", dict(n=1 << 31, D=8, M=4, bits=[2] * 4), EINVAL),
        ("M < 1", dict(n=300, D=8, M=0, bits=[2]), EINVAL),
        ("D % M", dict(n=300, D=8, M=3, bits=[2] * 3), EINVAL),
        ("max_iter < 1", dict(n=300, D=8, M=4, bits=[2] * 4, max_iter=0), EINVAL),
        ("bits 0", dict(n=300, D=8, M=4, bits=[2, 0, 2, 2]), EINVAL),
        ("bits 16", dict(n=300, D=8, M=4, bits=[2, 2, 2, 16]), EINVAL),
        ("more centres than rows", dict(n=300, D=8, M=4, bits=[2, 2, 9, 2]), EINVAL),
        ("more centres than the sample", dict(n=15, D=8, M=2, bits=[3, 4]), EINVAL),
        ("M > 128", dict(n=300, D=big_m, M=big_m, bits=[1] * big_m), EUNSUPPORTED),
        ("D > 4096", dict(n=300, D=4100, M=4, bits=[2] * 4), EUNSUPPORTED),
    ]
    for what, kw, want in cases:
        codes = []
        for fn, X, dev in forms:
            a = dict(kw)
            a.setdefault("X", X)
            codes.append(_call(fn, a["X"], a["n"], a["D"], a["M"], a["bits"], a.get("max_iter", 25),
                               a.get("cent", "out"), dev))
            assert vaqlib.vaqhip_last_error()
        assert codes == [want] * 4, (what, codes)
    # the refiner form: a null handle, and the timing call's null
    assert vaqlib.vaqhip_refiner_fit_codebooks(None, 4, (C.c_int * 4)(2, 2, 2, 2), None, 25, None, None, None) == EINVAL
    assert b"refiner is null" in vaqlib.vaqhip_last_error()
    assert vaqlib.vaqhip_last_fit_codebooks_timing(None) == EINVAL
    assert vaqlib.vaqhip_fit_codebooks_set_timing(1) == 0 and vaqlib.vaqhip_fit_codebooks_set_timing(0) == 0


def test_python_argument_checks():
    """a _u8 call takes a contiguous uint8 n x D array and nothing else: EINVAL before the library is reached; so are
    a bits list of the wrong length and an eigvec of the wrong shape"""
    import vaq_amd
    good = np.zeros((300, 8), np.uint8)
    for bad in (good.astype(np.float32), good[:, ::2], good[::2].T, np.zeros(8, np.uint8)):
        with pytest.raises(vaq_amd.VaqHipError) as e:
            vaq_amd.fit_codebooks_u8(bad, 4, [2] * 4)
        assert e.value.code == -1
    for kw in (dict(M=4, bits=[2] * 3), dict(M=3, bits=[2] * 3), dict(M=4, bits=[2] * 4, eigvec=np.eye(4, dtype=np.float32))):
        for fn, X in ((vaq_amd.fit_codebooks, good.astype(np.float32)), (vaq_amd.fit_codebooks_u8, good)):
            with pytest.raises(vaq_amd.VaqHipError) as e:
                fn(X, **kw)
            assert e.value.code == -1
    with pytest.raises(vaq_amd.VaqHipError) as e:
        vaq_amd.fit_codebooks(np.zeros(8, np.float32), 4, [2] * 4)
    assert e.value.code == -1


# ---- fit_codebooks_plan.h ------------------------------------------------------------------------------------------
def _build(tmp_path, name, extra=()):
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "vaq_amd", "csrc")] + list(extra) +
                          [os.path.join(ROOT, "tests", "cpp", "fit_codebooks_plan_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fit_codebooks_plan"), "fit_codebooks_plan_test")


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")


def test_plan_program(plan_exe):
    assert "fit_codebooks_plan_test: ok" in _run(plan_exe, "self")


def test_plan_program_under_sanitizers(tmp_path):
    """a plain executable with the sanitizers linked in, run directly"""
    exe = _build(tmp_path, "fit_codebooks_plan_test_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                                           "-fno-sanitize-recover=undefined"])
    assert "fit_codebooks_plan_test: ok" in _run(exe, "self")


@pytest.mark.parametrize("name", CASES)
def test_plan_of_every_case(plan_exe, name):
    """sample sizes, prefix lengths, run offsets, key width and halves as the restatement has them"""
    n, D, M, bits, kind, salt = cr.CASES[name]
    out = _run(plan_exe, "plan", n, ",".join(map(str, bits)))
    sample, n_pairs, n_runs, n_cent, k_max, key_bits, sampled = map(int, out[0].split())
    rows = [cr.sample_count(n, 1 << b) for b in bits]
    ks = [1 << b for b in bits]
    assert (sample, n_pairs, n_runs, n_cent, k_max, sampled) == (max(rows), sum(rows), 2 * sum(ks), sum(ks), max(ks), int(n > max(rows)))
    assert (1 << key_bits) >= n_runs > (1 << (key_bits - 1)) or (key_bits == 1 and n_runs <= 2)
    for s in range(M):
        k, r, half, run_off, cent_off, pair_off = map(int, out[1 + s].split())
        assert (k, r, half) == (ks[s], rows[s], (rows[s] + 1) // 2)
        assert (run_off, cent_off, pair_off) == (2 * sum(ks[:s]), sum(ks[:s]), sum(rows[:s]))


@pytest.mark.parametrize("name", CASES)
def test_plan_sources_of_every_case(plan_exe, name):
    """which source every subspace reads, and how long the gathered sample is, as the restatement has them"""
    n, D, M, bits, kind, salt = cr.CASES[name]
    out = _run(plan_exe, "plan", n, ",".join(map(str, bits)))
    sample, n_full, gather = map(int, out[1 + M].split())
    full = [int(v) for v in out[2 + M].split()]
    want = [int(not cr.sampled(n, 1 << b)) for b in bits]
    assert full == want and n_full == sum(want)
    assert sample == max([cr.sample_count(n, 1 << b) for b in bits if cr.sampled(n, 1 << b)], default=0)
    assert gather == int(sample > 0)


def test_permutation_head_of_the_program_is_the_restatement(plan_exe):
    for n, r in ((300, 16), (140000, 512), (131072, 512), (65536, 8)):
        got = np.array(_run(plan_exe, "head", n, r)[0].split(), np.int64)
        assert np.array_equal(got, cr.permutation_head(n, r))
