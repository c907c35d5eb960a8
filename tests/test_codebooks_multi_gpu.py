"""The sharded codebook fit on the GPU (vaqhip_multi_fit_codebooks[_u8], vaqhip_multi_refiner_fit_codebooks;
vaq_amd/csrc/vaqhip_multi_codebooks.cpp, the shard step in vaq_codebooks.hip): for every device list the single fit's
centres, iterations and NaN counts, bit for bit (NaN by position), against the centres recorded from the reference
(tests/golden/codebooks) and against vaqhip_fit_codebooks on device 0.  Multi-device cases are logical shards of
device 0.  The owner rule is s % G, so ownership is varied through G."""
import ctypes as C
import functools

import numpy as np
import pytest

import codebooks_ref as cr

pytestmark = pytest.mark.gpu

PATTERN = np.float32(7.25)
DEVICE_LISTS = ([0], [0] * 2, [0] * 3, [0] * 16)
FIXTURES = ("tiny", "odd", "sampled", "prefix", "bytes", "rotated", "mixed", "staged", "len1")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@functools.lru_cache(maxsize=None)
def inputs(name):
    return cr.make_inputs(name)


def sizes(D, M, bits):
    L = D // M
    ks = [1 << b for b in bits]
    return L, ks, np.concatenate([[0], np.cumsum(ks)]) * L


def out_arrays(D, M, bits):
    """(centres, iterations, nan rows), preset to patterns a refusal must leave"""
    L, ks, offs = sizes(D, M, bits)
    return np.full(int(offs[-1]), PATTERN, np.float32), np.full(M, -9, np.int32), np.full(M, -9, np.int32)


def split(cent, D, M, bits):
    L, ks, offs = sizes(D, M, bits)
    return [cent[offs[s]:offs[s + 1]].reshape(ks[s], L) for s in range(M)]


def single_fit(L_, X, M, bits, eig=None, max_iter=cr.MAX_ITER):
    n, D = X.shape
    cent, iters, nan = out_arrays(D, M, bits)
    fn = L_.vaqhip_fit_codebooks_u8 if X.dtype == np.uint8 else L_.vaqhip_fit_codebooks
    rc = fn(0, _p(X), n, D, M, (C.c_int * M)(*bits), _p(eig), max_iter, _p(cent), _p(iters), _p(nan))
    return rc, split(cent, D, M, bits), iters, nan


def sharded_fit(L_, devices, X, M, bits, eig=None, max_iter=cr.MAX_ITER):
    n, D = X.shape
    cent, iters, nan = out_arrays(D, M, bits)
    fn = L_.vaqhip_multi_fit_codebooks_u8 if X.dtype == np.uint8 else L_.vaqhip_multi_fit_codebooks
    rc = fn(len(devices), (C.c_int * len(devices))(*devices), _p(X), n, D, M, (C.c_int * M)(*bits), _p(eig), max_iter,
            _p(cent), _p(iters), _p(nan))
    return rc, split(cent, D, M, bits), iters, nan


def same_fit(got, want, what):
    from vaq_amd import _lib
    assert got[0] == 0, (what, _lib.load().vaqhip_multi_last_error())
    for s, (g, w) in enumerate(zip(got[1], want[1])):
        cr.assert_centres_equal(g, w, f"{what}, subspace {s}")
    assert np.array_equal(got[2], want[2]), f"{what}: iterations {got[2]} vs {want[2]}"
    assert np.array_equal(got[3], want[3]), f"{what}: NaN rows {got[3]} vs {want[3]}"


@functools.lru_cache(maxsize=None)
def fitted(name):
    """the single fit's answer on device 0 for a fixture case, computed once"""
    from vaq_amd import _lib
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = inputs(name)
    got = single_fit(_lib.load(), X, M, bits, eig)
    assert got[0] == 0
    return got


@functools.lru_cache(maxsize=None)
def rotated_sampled(byte_valued):
    """70000 x 16, M 4, bits {8,5,4,3}, a random orthogonal eigvec in front: rotation and sampling together"""
    rng = np.random.default_rng(4242 + int(byte_valued))
    n, D = 70000, 16
    eig = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(D, D)))[0], np.float32)
    if byte_valued:
        X = rng.integers(0, 256, size=(n, D), dtype=np.int64).astype(np.uint8)
    else:
        X = (rng.normal(size=(n, D)) * 4).astype(np.float32)
    return X, eig, 4, (8, 5, 4, 3)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_at_every_device_list(vaqlib, name):
    """Every recorded case through the sharded call at G = 1, 2, 3, 16: the fixture's centres, iter_count and NaN
    centres, and the single fit's.  `mixed`: one owner needs all rows while the others take the sample; `prefix`: two
    owners take different prefixes of one sample; G = 16 over M <= 4 leaves owners idle."""
    n, D, M, bits, kind, salt = cr.CASES[name]
    fx = cr.load_fixture(name)
    X, eig = inputs(name)
    want = fitted(name)
    for devices in DEVICE_LISTS:
        got = sharded_fit(vaqlib, devices, X, M, bits, eig)
        same_fit(got, want, f"{name} over {len(devices)} shards")
        for s in range(M):
            cr.assert_centres_equal(got[1][s], fx["centres_%d" % s], f"{name} over {len(devices)} shards, subspace {s}")
            assert got[2][s] == int(fx["iterations_%d" % s]) and got[3][s] == int(fx["nan_rows_%d" % s].sum())


@pytest.mark.parametrize("byte_valued", [False, True])
def test_rotation_and_sampling_together(vaqlib, byte_valued):
    """No fixture has both: the shard step projects only the sample rows a shard holds, per owner only its columns."""
    X, eig, M, bits = rotated_sampled(byte_valued)
    want = single_fit(vaqlib, X, M, bits, eig)
    assert want[0] == 0
    assert not np.array_equal(want[1][0], single_fit(vaqlib, X, M, bits, None)[1][0])  # (the rotation matters)
    for G in (2, 3):
        same_fit(sharded_fit(vaqlib, [0] * G, X, M, bits, eig), want, f"rotated and sampled over {G} shards")


def test_refiner_form(vaqlib):
    """Float rows and byte rows resident in a multi refiner, read in place: a last shard grown by add_rows[_u8], an
    empty shard (N < G), with and without eigvec -- each equals vaqhip_refiner_fit_codebooks over the same rows."""
    import vaq_amd

    def one_device(X, M, bits, eig):
        r = vaq_amd.VaqRefiner(X.shape[1])
        (r.set_rows_u8 if X.dtype == np.uint8 else r.set_rows)(X)
        out = r.fit_codebooks(M, bits, eig)
        r.close()
        return (0,) + tuple(out)

    Xr, eig, M, bits = rotated_sampled(False)
    X8 = rotated_sampled(True)[0]
    n, D = Xr.shape
    for X, E in ((Xr, eig), (X8, eig), (X8, None)):
        want = one_device(X, M, bits, E)
        r = vaq_amd.VaqMultiRefiner([0, 0, 0], D)
        if E is eig and X is Xr:
            with pytest.raises(vaq_amd.VaqHipError) as e:
                r.fit_codebooks(M, bits)
            assert e.value.code == -7  # ESTATE: no rows yet
        u8 = X.dtype == np.uint8
        (r.set_rows_u8 if u8 else r.set_rows)(X[:30000])
        (r.add_rows_u8 if u8 else r.add_rows)(X[30000:])
        assert r.info()["shard_rows"] == [10000, 10000, 50000]
        same_fit((0,) + tuple(r.fit_codebooks(M, bits, E)), want, f"refiner, grown last shard, {X.dtype}, eigvec {E is not None}")
        with pytest.raises(vaq_amd.VaqHipError) as e:
            r.fit_codebooks(3, (2, 2, 2))  # (the adapter's own refusal; the C call's: test_refusals_leave_the_outputs)
        assert e.value.code == -1
        r.close()
    # `mixed` through the refiner: one owner reads all rows of its columns from every shard
    n, D, M, bits, kind, salt = cr.CASES["mixed"]
    r = vaq_amd.VaqMultiRefiner([0, 0], D)
    r.set_rows(inputs("mixed")[0])
    same_fit((0,) + tuple(r.fit_codebooks(M, bits)), fitted("mixed"), "refiner, mixed")
    r.close()
    # N < G: shards without rows
    n, D, M, bits, kind, salt = cr.CASES["tiny"]
    X = inputs("tiny")[0][:20]
    r = vaq_amd.VaqMultiRefiner([0] * 16, D)
    r.set_rows(X[:9])
    assert r.info()["shard_rows"][9:] == [0] * 7
    r.add_rows(X[9:])
    same_fit((0,) + tuple(r.fit_codebooks(M, (1, 2, 3, 4))), one_device(X, M, (1, 2, 3, 4), None), "refiner, N < G")
    r.set_rows(X[:17])
    assert r.info()["shard_rows"] == [2] * 8 + [1] + [0] * 7
    same_fit((0,) + tuple(r.fit_codebooks(M, (1, 2, 3, 4))), one_device(X[:17], M, (1, 2, 3, 4), None), "refiner, empty shards")
    r.close()


@pytest.mark.parametrize("name", ["mixed", "prefix"])
def test_ownership_changes_nothing(vaqlib, name):
    """The owner rule is s % G: G = 2 and G = 3 give every subspace another owner and other neighbours in its owner's
    batch, and the same centres."""
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = inputs(name)
    two, three = sharded_fit(vaqlib, [0] * 2, X, M, bits, eig), sharded_fit(vaqlib, [0] * 3, X, M, bits, eig)
    same_fit(two, three, f"{name}: G = 2 against G = 3")
    same_fit(two, fitted(name), name)


def test_refusals_leave_the_outputs(vaqlib):
    """Before any device is touched, and after the run: a row of FLT_MAX values has no centre in reach on its owner."""
    import vaq_amd
    n, D, M, bits, kind, salt = cr.CASES["odd"]
    X, _ = inputs("odd")
    err = vaqlib.vaqhip_multi_last_error

    def untouched(got):
        return all(np.all(c == PATTERN) for c in got[1]) and np.all(got[2] == -9) and np.all(got[3] == -9)

    for devices, mm, bb, it, code, text in (([0, 0], M, (5, 16), 25, -1, b"bits[1]=16"), ([0, 0], M, (13, 3), 25, -1, b"centres from"),
                                            ([0, 0], M, bits, 0, -1, b"max_iter=0"), ([0] * 17, M, bits, 25, -1, b"n_devices=17"),
                                            ([0, 0], 5, (2,) * 5, 25, -1, b"equal length")):
        cent, iters, nan = out_arrays(D, M, bits)
        rc = vaqlib.vaqhip_multi_fit_codebooks(len(devices), (C.c_int * len(devices))(*devices), _p(X), n, D, mm,
                                               (C.c_int * mm)(*bb), None, it, _p(cent), _p(iters), _p(nan))
        assert rc == code and text in err(), (rc, err())
        assert untouched((rc, [cent], iters, nan))
    cent, iters, nan = out_arrays(D, M, bits)
    assert vaqlib.vaqhip_multi_fit_codebooks(0, None, _p(X), n, D, M, (C.c_int * M)(*bits), None, 25, _p(cent), _p(iters), _p(nan)) == -1
    assert vaqlib.vaqhip_multi_refiner_fit_codebooks(None, M, (C.c_int * M)(*bits), None, 25, _p(cent), _p(iters), _p(nan)) == -1
    assert untouched((0, [cent], iters, nan))
    # the refiner form's own refusals, at the C ABI: no rows yet (ESTATE), then M not dividing the REFINER's D (the single
    # fit's refusal with its text), bits out of range and max_iter -- the outputs untouched each time
    r = vaq_amd.VaqMultiRefiner([0, 0, 0], D)

    def refiner_fit(mm, bb, it=25):
        cent, iters, nan = out_arrays(D, M, bits)
        rc = vaqlib.vaqhip_multi_refiner_fit_codebooks(r._h, mm, (C.c_int * mm)(*bb), None, it, _p(cent), _p(iters), _p(nan))
        assert untouched((rc, [cent], iters, nan))
        return rc

    assert refiner_fit(M, bits) == -7 and b"holds no rows" in err()
    assert refiner_fit(5, (2,) * 5) == -7  # (the state is refused first)
    r.set_rows(X)
    assert D % 5 != 0 and refiner_fit(5, (2,) * 5) == -1 and b"D=24 is not M=5 subspaces of equal length" in err()
    assert refiner_fit(M, (5, 16)) == -1 and b"bits[1]=16" in err()
    assert refiner_fit(M, bits, it=0) == -1 and b"max_iter=0" in err()
    r.close()
    bad = X.copy()
    bad[17, :] = np.finfo(np.float32).max  # (x - mean)^2 overflows: no distance is below FLT_MAX
    for devices in ([0, 0], [0] * 3):
        got = sharded_fit(vaqlib, devices, bad, M, bits)
        assert got[0] == -1 and b"row -1" in err()
        assert untouched(got)
    assert single_fit(vaqlib, bad, M, bits)[0] == -1  # (as the single fit)
    r = vaq_amd.VaqMultiRefiner([0, 0], D)
    r.set_rows(bad)
    cent, iters, nan = out_arrays(D, M, bits)
    rc = vaqlib.vaqhip_multi_refiner_fit_codebooks(r._h, M, (C.c_int * M)(*bits), None, 25, _p(cent), _p(iters), _p(nan))
    assert rc == -1 and b"row -1" in err() and untouched((rc, [cent], iters, nan))
    r.close()


def test_a_shard_that_fails_in_setup_takes_the_run_down_cleanly(vaqlib):
    """[0, 977]: shard 0 opens its stream, uploads its rows and succeeds in setup; shard 1 is refused by hipSetDevice (an
    error return: ordinal 977 does not exist).  The run's teardown (vaq_amd/csrc/vaqhip_shard_run.h) then has one
    opened and one unopened shard: ENODEVICE naming shard 1, the outputs untouched, the caller's device as it was, and
    the next fit of the same rows is the single fit's."""
    import torch
    rng = np.random.default_rng(977)
    X = (rng.normal(size=(64, 4)) * 5).astype(np.float32)
    M, bits = 4, (1, 2, 3, 4)
    torch.cuda.set_device(torch.cuda.device_count() - 1)
    dev = torch.cuda.current_device()
    got = sharded_fit(vaqlib, [0, 977], X, M, bits)
    assert got[0] == -3 and vaqlib.vaqhip_multi_last_error().startswith(b"shard 1 (device 977): ")
    assert all(np.all(c == PATTERN) for c in got[1]) and np.all(got[2] == -9) and np.all(got[3] == -9)
    assert torch.cuda.current_device() == dev
    torch.cuda.set_device(0)
    want = single_fit(vaqlib, X, M, bits)
    assert want[0] == 0
    same_fit(sharded_fit(vaqlib, [0, 0], X, M, bits), want, "after the failed setup")


def test_python_adapters_and_timing(vaqlib):
    import vaq_amd
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = inputs("rotated")
    same_fit((0,) + tuple(vaq_amd.fit_codebooks(X, M, bits, eig, devices=[0, 0, 0])), fitted("rotated"), "fit_codebooks(devices=)")
    t = vaq_amd.last_multi_fit_codebooks_timing()
    assert t["n_devices"] == 3 and t["owner_subspaces"] == [2, 1, 1] and sum(t["owner_subspaces"]) == M
    assert t["rows"] == n and t["dims"] == D and t["subspaces"] == M and t["sample_rows"] == n
    assert t["iterations"] == max(fitted("rotated")[2]) and t["total_ms"] > 0 and t["assign_ms"] == 0
    vaq_amd.fit_codebooks_timing(True)
    try:
        same_fit((0,) + tuple(vaq_amd.fit_codebooks(X, M, bits, eig, devices=[0, 0])), fitted("rotated"), "with phase times")
        t = vaq_amd.last_multi_fit_codebooks_timing()
        assert t["owner_subspaces"] == [2, 2] and t["assign_ms"] > 0 and t["accumulate_ms"] > 0 and t["update_ms"] > 0
    finally:
        vaq_amd.fit_codebooks_timing(False)
    X8 = inputs("bytes")[0]
    n, D, M, bits, kind, salt = cr.CASES["bytes"]
    same_fit((0,) + tuple(vaq_amd.fit_codebooks_u8(X8, M, bits, devices=[0] * 16)), fitted("bytes"), "fit_codebooks_u8(devices=)")
    t = vaq_amd.last_multi_fit_codebooks_timing()
    assert t["n_devices"] == 16 and t["owner_subspaces"] == [1] * 4 + [0] * 12
    same_fit((0,) + tuple(vaq_amd.fit_codebooks_u8(X8, M, bits, devices=[0])), fitted("bytes"), "one device")
    t = vaq_amd.last_multi_fit_codebooks_timing()
    assert t["n_devices"] == 1 and t["owner_subspaces"] == [M]
    r = vaq_amd.VaqMultiRefiner([0, 0], D)
    r.set_rows_u8(X8)
    same_fit((0,) + tuple(r.fit_codebooks(M, bits)), fitted("bytes"), "VaqMultiRefiner.fit_codebooks")
    r.close()


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/fit_codebooks_multi_shim_test.cpp: VaqHip::fitCodebooks and fitCodebooksRefineDataset after
    setDevices({0, 0, 0}) give the single device's centres"""
    import os
    import subprocess
    from vaq_amd import build
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = inputs("rotated")
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([n, D, M], np.int32).tobytes())
        f.write(np.array(bits, np.int32).tobytes())
        f.write(eig.tobytes())
        f.write(X.tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fit_codebooks_multi_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "fit_codebooks_multi_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fit_codebooks_multi_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_takes_the_sharded_route(vaqlib, tmp_path):
    """demo_vaqhip --fit-codebooks --devices 0,0 --refine-resident --encode: the saved centres are the single-device
    run's file byte for byte, and so are the codes"""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = inputs("rotated")
    io.write_vecs(str(tmp_path / "base.fvecs"), X)
    io.write_vecs(str(tmp_path / "q.fvecs"), X[:9] + np.float32(0.125))
    eig.tofile(str(tmp_path / "eig.f32"))
    files = {}
    for tag, extra in (("one", []), ("many", ["--devices", "0,0", "--refine-resident"])):
        r = subprocess.run([exe, "--fit-codebooks", "--encode", "--bits", ",".join(map(str, bits)), "--dataset", str(tmp_path / "base.fvecs"),
                            "--eigen", str(tmp_path / "eig.f32"), "--timeseries-size", str(D), "--queries", str(tmp_path / "q.fvecs"),
                            "--k", "5", "--save", str(tmp_path / (tag + "_c.bin")), "--save-enc", str(tmp_path / (tag + "_cb.bin")),
                            "--result", str(tmp_path / (tag + ".csv"))] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        files[tag] = r.stdout
    assert "across 2 shards: fit" in files["many"] and "subspaces per owner 2 2" in files["many"]
    assert "from the resident rows" in files["many"]
    for name in ("_c.bin", "_cb.bin", ".csv"):
        assert (tmp_path / ("one" + name)).read_bytes() == (tmp_path / ("many" + name)).read_bytes(), name
    got = io.load_centroids(str(tmp_path / "many_c.bin"))
    for s in range(M):
        cr.assert_centres_equal(got[s], fitted("rotated")[1][s], f"demo, subspace {s}")


def test_end_to_end_sharded_fit_encode_search(vaqlib):
    """`rotated`: multi refiner -> sharded fit -> vaqhip_multi_create -> vaqhip_multi_encode_from_refiner -> search,
    against the single-device fit -> vaqhip_encode -> search: equal codes, labels and distances."""
    import vaq_amd
    from vaq_amd.index import VaqHipMulti
    n, D, M, bits, kind, salt = cr.CASES["rotated"]
    X, eig = inputs("rotated")
    k, Q = 10, X[:37] + np.float32(0.125)
    r = vaq_amd.VaqMultiRefiner([0, 0], D)
    r.set_rows(X)
    cents, iters, nan = r.fit_codebooks(M, bits, eig)
    assert not nan.any()
    m = VaqHipMulti([0, 0], list(bits), cents, eig=eig)
    codes = m.encode_from_refiner(r, return_codes=True)
    many = m.search(Q, k)
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = [np.ascontiguousarray(c) for c in fitted("rotated")[1]]
    v.mEigenVectors = eig
    v.encode(X, projected=False)
    one = v.search(Q, k)
    assert np.array_equal(codes, v.mCodebook)
    assert np.array_equal(many.labels.reshape(-1, k), one.labels.reshape(-1, k))
    assert np.array_equal(many.distances.view(np.uint32).reshape(-1, k), one.distances.view(np.uint32).reshape(-1, k))
    for x in (m, r, v):
        x.close()
