"""Building a queryLUT index across the shards of a multi-device index on the GPU: the sharded quantile fit
(vaqhip_multi_lut_fit_quantiles, vaqhip_multi_refiner_lut_fit_quantiles; vaq_amd/csrc/vaqhip_multi_lutfit.cpp, the
column kernel in vaq_lutfit.hip), Q on the shards (vaqhip_multi_set_lut_quantiles) and the engine's encoder across them
(vaqhip_multi_encode_lut_*).

Logical shards of device 0 ([0] * G) exercise every path on one GPU.  Every comparison is on bit patterns (uint32 view,
array_equal): the sharded fit against the single vaqhip_lut_fit_quantiles and the numpy restatement
(tests/lutfit_ref.py), the sharded encoder against vaqhip_encode_lut.  There is no tolerance anywhere: a sorted column
does not depend on how its values were cut, and a row's code depends on that row alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import lutfit_ref as lr
import seq_exact_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
DEVICE_LISTS = ([0], [0, 0], [0, 0, 0], [0] * 8)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    bad = np.argwhere(u32(got) != u32(want))
    assert bad.size == 0, f"{what}: {len(bad)} differ, first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def single_fit(vaqlib, X, bits, eig=None):
    """vaqhip_lut_fit_quantiles: (rc, centroidsMat 256 x D, Q D x 257); the outputs start as a pattern"""
    X = np.ascontiguousarray(X, np.float32)
    D = X.shape[1]
    cent = np.full((D, 256), SENTINEL, np.float32)
    q = np.full((D, 257), SENTINEL, np.float32)
    rc = vaqlib.vaqhip_lut_fit_quantiles(0, _p(X), X.shape[0], D, (C.c_int * D)(*bits), _p(eig), _p(cent), _p(q))
    return rc, np.ascontiguousarray(cent.T), q


def multi_fit(vaqlib, devs, X, bits, eig=None):
    X = np.ascontiguousarray(X, np.float32)
    D = X.shape[1]
    cent = np.full((D, 256), SENTINEL, np.float32)
    q = np.full((D, 257), SENTINEL, np.float32)
    rc = vaqlib.vaqhip_multi_lut_fit_quantiles(len(devs), (C.c_int * len(devs))(*devs), _p(X), X.shape[0], D,
                                               (C.c_int * D)(*bits), _p(eig), _p(cent), _p(q))
    return rc, np.ascontiguousarray(cent.T), q


def check_against_single(vaqlib, X, bits, device_lists, eig=None, what="", restated=None):
    rc, want_c, want_q = single_fit(vaqlib, X, bits, eig)
    assert rc == 0, vaqlib.vaqhip_last_error()
    if restated is not None:
        same_bits(want_q, restated[1], f"{what}: single fit against the restatement, quantiles")
        same_bits(want_c, restated[0], f"{what}: single fit against the restatement, centres")
    for devs in device_lists:
        rc, cent, Qs = multi_fit(vaqlib, devs, X, bits, eig)
        assert rc == 0, (what, devs, vaqlib.vaqhip_multi_last_error())
        same_bits(Qs, want_q, f"{what} G={len(devs)} quantiles")
        same_bits(cent, want_c, f"{what} G={len(devs)} centres")
    return want_c, want_q


@pytest.mark.parametrize("name", lr.FIT_CASES)
def test_fit_equals_restatement_and_single_fit(vaqlib, name):
    X, bits = lr.fit_case(name)
    check_against_single(vaqlib, X, bits, DEVICE_LISTS, what=name, restated=lr.fit_ref(name))
    import vaq_amd
    t = vaq_amd.last_lut_fit_multi_timing()  # the last fit of this thread: [0] * 8
    assert t["rows"] == X.shape[0] and t["dims"] == X.shape[1] and t["n_devices"] == 8
    assert t["total_ms"] > 0 and t["sort_ms"] > 0 and t["columns_ms"] > 0 and t["means_ms"] > 0


def _shape_cases():
    rng = np.random.default_rng(2024)
    cases = {}
    # empty shards: the cut of 1 and of 5 rows over 8 (5 = 1 + 1 + 1 + 1 + 1 + 0 + 0 + 0)
    cases["n1_G8"] = (np.array([[1.5, -2.25, 0.0]], np.float32), [1, 3, 8], ([0] * 8,))
    cases["n5_G8"] = ((rng.normal(size=(5, 3)) * 4).astype(np.float32), [2, 8, 1], ([0] * 8,))
    # idle owners (D < G) and a partial last round (5 = 3 + 2)
    cases["D2_G8"] = ((rng.normal(size=(300, 2)) * 4).astype(np.float32), [8, 3], ([0] * 8,))
    cases["D5_G3"] = ((rng.normal(size=(300, 5)) * 4).astype(np.float32), [8, 5, 3, 2, 1], ([0] * 3,))
    # tile edges: 256 rows per workgroup of the column kernel, 2048 values per tile of the means kernel (bits = 1
    # puts about half of 4099 values into one bucket)
    for n in (255, 256, 257, 4099):
        cases[f"n{n}"] = ((rng.normal(size=(n, 3)) * 9).astype(np.float32), [1, 8, 4], ([0], [0] * 3))
    cases["bits_1_and_8"] = ((rng.normal(size=(1000, 6)) * 3).astype(np.float32), [1, 8, 1, 8, 8, 1], ([0, 0], [0] * 8))
    const = np.empty((1000, 3), np.float32)
    const[:] = np.array([3.7, -1e-3, 1e30], np.float32)  # Q not monotone once rounded
    cases["const"] = (const, [4, 8, 6], ([0, 0], [0] * 3))
    # -0 on the first shard, +0 on the second: -0 sorts first wherever it came from
    zeros = np.zeros((600, 2), np.float32)
    zeros[:300, 0] = -0.0
    zeros[300:, 1] = -0.0
    zeros[::5] += rng.normal(size=(120, 2)).astype(np.float32)
    cases["signed_zeros"] = (zeros, [3, 8], ([0, 0], [0] * 3))
    # equal values on both sides of every cut: 12 rows over 2, 3 and 4 shards cut at 6; 4, 8; 3, 6, 9
    eq = np.repeat(np.array([[1.0], [2.0], [2.0], [2.0], [5.0], [5.0]], np.float32), 2, axis=0)
    eq = np.concatenate([eq, -eq], axis=1)
    cases["equal_across_cuts"] = (np.ascontiguousarray(eq), [2, 3], ([0] * 2, [0] * 3, [0] * 4))
    return cases


SHAPE_CASES = _shape_cases()


@pytest.mark.parametrize("name", sorted(SHAPE_CASES))
def test_fit_shapes(vaqlib, name):
    X, bits, device_lists = SHAPE_CASES[name]
    check_against_single(vaqlib, X, bits, device_lists, what=name, restated=lr.fit(X, bits))


def test_signed_zero_case_holds_both_zeros():
    X = SHAPE_CASES["signed_zeros"][0]
    for col in (0, 1):
        first, second = X[:300, col], X[300:, col]
        assert (np.signbit(first) & (first == 0)).any() != (np.signbit(second) & (second == 0)).any()


@pytest.mark.parametrize("D,n,device_lists", [(128, 4099, ([0], [0] * 3)), (20, 1000, ([0], [0] * 3, [0] * 16))])
def test_fit_projection(vaqlib, D, n, device_lists):
    """eigvec != NULL.  D = 128, n = 4099: the single fit projects with project_tile_kernel; D = 20: with project_kernel.
    The fused column kernel gives the same values either way.  [0] * 16 at D = 20: a full round of 16 columns, then a
    partial one of 4."""
    rng = np.random.default_rng(D)
    X = (rng.normal(size=(n, D)) * rng.uniform(0.5, 20, size=D)).astype(np.float32)
    eig = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32))
    bits = [int(b) for b in rng.integers(1, 9, size=D)]
    check_against_single(vaqlib, X, bits, device_lists, eig=eig, what=f"projected D={D}")


def test_fit_refuses_non_finite_values(vaqlib):
    X, bits = lr.fit_case("n4099_d5")
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[-1, 3] = bad  # the last row of the last shard
        rc, cent, Qs = multi_fit(vaqlib, [0] * 3, Xb, bits)
        assert rc == -1 and b"NaN or infinite" in vaqlib.vaqhip_multi_last_error()
        assert np.all(cent == SENTINEL) and np.all(Qs == SENTINEL)
    # finite rows, an infinity only the projection produces: 3e38 + 3e38
    Xb = X[:700].copy()
    Xb[350, :] = 0
    Xb[350, :2] = 3e38
    eig = np.zeros((5, 5), np.float32)
    eig[:, :] = np.eye(5, dtype=np.float32)
    eig[1, 0] = 1.0
    assert np.all(np.isfinite(Xb))
    rc, cent, Qs = multi_fit(vaqlib, [0] * 3, Xb, bits, eig)
    assert rc == -1 and b"after the projection" in vaqlib.vaqhip_multi_last_error()
    assert np.all(cent == SENTINEL) and np.all(Qs == SENTINEL)
    rc, _, _ = single_fit(vaqlib, Xb, bits, eig)
    assert rc == -1  # the single fit refuses the same rows
    rc, cent, Qs = multi_fit(vaqlib, [0] * 3, X, bits)  # and the next fit is sound
    assert rc == 0
    same_bits(cent, lr.fit_ref("n4099_d5")[0], "the fit after the refusals")


def test_a_shard_that_fails_in_setup_takes_the_run_down_cleanly(vaqlib):
    """[0, 977]: shard 0 opens its stream, uploads its rows and succeeds in setup; shard 1 is refused by hipSetDevice (an
    error return: ordinal 977 does not exist).  The run's teardown (vaq_amd/csrc/vaqhip_shard_run.h) then has one
    opened and one unopened shard: ENODEVICE naming shard 1, the outputs untouched, the caller's device as it was, and
    the next fit of the same rows is the single fit's."""
    import torch
    rng = np.random.default_rng(977)
    X = (rng.normal(size=(64, 4)) * 5).astype(np.float32)
    bits = [3, 8, 1, 5]
    torch.cuda.set_device(torch.cuda.device_count() - 1)
    dev = torch.cuda.current_device()
    rc, cent, Qs = multi_fit(vaqlib, [0, 977], X, bits)
    assert rc == -3 and vaqlib.vaqhip_multi_last_error().startswith(b"shard 1 (device 977): ")
    assert np.all(cent == SENTINEL) and np.all(Qs == SENTINEL)
    assert torch.cuda.current_device() == dev
    torch.cuda.set_device(0)
    check_against_single(vaqlib, X, bits, ([0, 0],), what="after the failed setup")


def test_fit_refiner_form(vaqlib):
    """set_rows over [0, 0, 0], then add_rows growing the last shard: the cut is the refiner's, the result the single
    fit's over the concatenated rows; with and without eigvec.  A refiner without rows: ESTATE."""
    import vaq_amd
    X, bits = lr.fit_case("n4099_d5")
    rng = np.random.default_rng(5)
    eig = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(5, 5)))[0].astype(np.float32))
    r = vaq_amd.VaqMultiRefiner([0, 0, 0], 5)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        r.fit_quantiles(bits)
    assert e.value.code == -7
    r.set_rows(X[:3000], id_base=11)
    r.add_rows(X[3000:])
    assert r.info()["shard_rows"] == [1000, 1000, 2099]
    for E in (None, eig):
        rc, want_c, want_q = single_fit(vaqlib, X, bits, E)
        assert rc == 0
        cent, q = r.fit_quantiles(bits, E)
        same_bits(q, want_q, "refiner form quantiles")
        same_bits(np.ascontiguousarray(cent.T), want_c, "refiner form centres")
    # an empty shard in the middle of the list: 2 rows over 3 shards are cut 1 + 1 + 0, the append grows the empty one
    r.set_rows(X[:2])
    r.add_rows(X[2:50])
    assert r.info()["shard_rows"] == [1, 1, 48]
    r.set_rows(X[:1])
    assert r.info()["shard_rows"] == [1, 0, 0]
    cent, q = r.fit_quantiles(bits)
    rc, want_c, want_q = single_fit(vaqlib, X[:1], bits)
    same_bits(q, want_q, "refiner form, empty shards")
    same_bits(np.ascontiguousarray(cent.T), want_c, "refiner form, empty shards")
    r.close()


def test_python_adapters_route_to_the_sharded_fit(vaqlib):
    import vaq_amd
    X, bits = lr.fit_case("grid")
    want_c, want_q = lr.fit_ref("grid")
    cent, q = vaq_amd.lut_fit_quantiles_multi([0, 0], X, bits)
    same_bits(q, want_q, "lut_fit_quantiles_multi")
    same_bits(np.ascontiguousarray(cent.T), want_c, "lut_fit_quantiles_multi")
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(bits)
    v.fitQuantiles(X, devices=[0, 0, 0])
    same_bits(v.centroidsMat, want_c, "fitQuantiles(devices=)")
    same_bits(v.mQuantiles, want_q, "fitQuantiles(devices=)")
    assert [c.shape for c in v.mCentroidsPerSubs] == [(1 << b, 1) for b in bits]
    v.close()


# ---- the engine's encoder across the shards ----
@functools.lru_cache(maxsize=None)
def encoder_case(projected):
    """projected = 1: the integer grid under the restatement's fit, the rows are the finite probes (every Q[q], values
    midway between centres, values outside the training range).  projected = 0: gaussian rows and a rotation, the fit
    that of the rotated rows."""
    if projected:
        X, bits = lr.fit_case("grid")
        cent, Qs = lr.fit_ref("grid")
        P = lr.probes("grid")
        rows = np.ascontiguousarray(P[np.isfinite(P).all(axis=1)])
        queries = np.random.default_rng(3).integers(-4, 5, size=(21, 4)).astype(np.float32)
        return dict(bits=list(bits), cent=cent, Qs=Qs, eig=None, rows=rows, queries=queries)
    X, bits = lr.fit_case("n4099_d5")
    rng = np.random.default_rng(5)
    eig = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(5, 5)))[0].astype(np.float32))
    return dict(bits=list(bits), cent=None, Qs=None, eig=eig, rows=np.ascontiguousarray(X[:1500]),
                queries=(rng.normal(size=(21, 5)) * 8).astype(np.float32))


def encoder_fit(vaqlib, c):
    if c["cent"] is None:
        rc, c["cent"], c["Qs"] = single_fit(vaqlib, lr.fit_case("n4099_d5")[0], c["bits"], c["eig"])
        assert rc == 0
    return c


def seq_single(c):
    import vaq_amd
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = c["bits"]
    v.mCentroidsPerSubs = sr.centroid_list(c["bits"], c["cent"])
    v.mEigenVectors = c["eig"]
    v.mQuantiles = c["Qs"]
    return v


def seq_multi(c, G):
    from vaq_amd.index import VaqHipMulti
    return VaqHipMulti([0] * G, c["bits"], sr.centroid_list(c["bits"], c["cent"]), c["eig"], sequential_sum=True)


def same_state_and_answers(a, b, queries, what):
    ia, ib = a.info(), b.info()
    for key in ("N", "id_base", "shard_rows", "n_devices"):
        assert ia[key] == ib[key], (what, key, ia[key], ib[key])
    for m in (a, b):
        m.set_option("exact_ties", 1)
    for k in (1, 10):
        ra, rb = a.search(queries, k), b.search(queries, k)
        assert np.array_equal(ra.labels, rb.labels), (what, k)
        assert np.array_equal(u32(ra.distances), u32(rb.distances)), (what, k)


@pytest.mark.parametrize("projected", [0, 1])
@pytest.mark.parametrize("G", [1, 2, 3])
def test_encode_lut_across_shards(vaqlib, G, projected):
    """set, add and from_refiner: codes_out is vaqhip_encode_lut's matrix, shard_rows / N / id_base and the exact_ties
    answers at k = 1 and 10 are those of a multi index loaded with the single encoder's codes."""
    import vaq_amd
    c = encoder_fit(vaqlib, encoder_case(projected))
    rows, n1 = c["rows"], c["rows"].shape[0] - 301
    v = seq_single(c)
    v.encodeLUT(rows, projected=bool(projected))
    want = np.array(v.mCodebook)
    a, b = seq_multi(c, G), seq_multi(c, G)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        a.encode_lut(rows, projected=bool(projected))
    assert e.value.code == -7  # VAQHIP_ESTATE: no Q yet
    a.set_lut_quantiles(c["Qs"])
    with pytest.raises(vaq_amd.VaqHipError) as e:
        a.encode_lut_add(rows[:5], projected=bool(projected))
    assert e.value.code == -7  # no codes yet
    got = a.encode_lut(rows[:n1], projected=bool(projected), id_base=7, return_codes=True)
    assert np.array_equal(got, want[:n1])
    b.set_codes(want[:n1], id_base=7)
    same_state_and_answers(a, b, c["queries"], ("set", G, projected))
    got = a.encode_lut_add(rows[n1:], projected=bool(projected), return_codes=True)
    assert np.array_equal(got, want[n1:])
    b.add_codes(want[n1:])
    same_state_and_answers(a, b, c["queries"], ("add", G, projected))
    t = a.last_encode_timing()
    assert t["rows"] == 301 and t["n_devices"] == G and t["encode_ms"] > 0
    if not projected or c["eig"] is None:  # the refiner holds RAW rows: the call encodes with projected = 0
        r = vaq_amd.VaqMultiRefiner([0] * G, len(c["bits"]))
        r.set_rows(rows[:n1], id_base=7)
        r.add_rows(rows[n1:])
        assert a.encode_lut(rows[:3], projected=bool(projected)) is None  # (something else in between)
        got = a.encode_lut_from_refiner(r, return_codes=True)
        assert np.array_equal(got, want)
        same_state_and_answers(a, b, c["queries"], ("from_refiner", G, projected))
        r.close()
    for x in (a, b, v):
        x.close()


def test_the_two_encoders_differ_where_the_issue_says(vaqlib):
    """VAQ::encode's rule (first global argmin) and the engine's differ on a row above the training range and on a value
    exactly half-way between two centres -- otherwise the encoder test above would show nothing encode() would not."""
    c = encoder_fit(vaqlib, encoder_case(1))
    rows, bits, cent, Qs = c["rows"], c["bits"], c["cent"], c["Qs"]
    a = seq_multi(c, 2)
    a.set_lut_quantiles(Qs)
    lut = a.encode_lut(rows, projected=True, return_codes=True)
    plain = a.encode(rows, projected=True, return_codes=True)
    v = seq_single(c)
    v.encodeLUT(rows, projected=True)
    assert np.array_equal(lut, v.mCodebook)
    d, N = 0, 1 << bits[0]
    x, cc = rows[:, d], cent[:N, d]
    above = x > Qs[d, N]
    mids = np.unique(((cc[:-1] + cc[1:]) / np.float32(2))[cc[:-1] != cc[1:]])
    midway = np.isin(x, mids) & (x >= Qs[d, 0]) & (x <= Qs[d, N])
    assert above.any() and midway.any()
    assert np.all(lut[above, d] != plain[above, d])
    assert np.all(lut[midway, d] != plain[midway, d])
    a.close(), v.close()


def test_set_lut_quantiles_checks(vaqlib):
    import vaq_amd
    from vaq_amd.index import VaqHipMulti
    c = encoder_fit(vaqlib, encoder_case(1))
    plain = VaqHipMulti([0, 0], [8] * 4, [np.zeros((256, 1), np.float32)] * 4)
    with pytest.raises(vaq_amd.VaqHipError) as e:
        plain.set_lut_quantiles(np.zeros((4, 257), np.float32))
    assert e.value.code == -1  # not sequential-sum shards
    plain.close()
    a = seq_multi(c, 2)
    q = c["Qs"].copy()
    q[1, 2] = np.nan
    with pytest.raises(vaq_amd.VaqHipError) as e:
        a.set_lut_quantiles(q)
    assert e.value.code == -1
    with pytest.raises(vaq_amd.VaqHipError) as e:
        a.encode_lut(c["rows"])
    assert e.value.code == -7  # the refused Q was not taken
    a.set_lut_quantiles(c["Qs"])
    a.set_lut_quantiles(c["Qs"])  # idempotent
    a.close()


def test_end_to_end_sharded_build_and_exact_search(vaqlib):
    """fit across [0, 0] from a refiner's rows -> multi index with the centres -> Q -> encode_lut_from_refiner -> search
    with exact_ties: seq_exact_ref's answer over the restatement's centres and codes slot for slot, which is the
    single-device build's (test_lutfit_gpu.py::test_end_to_end_build_and_exact_search)."""
    import vaq_amd
    from vaq_amd.index import VaqHipMulti
    X, bits = lr.fit_case("grid")
    k = 10
    queries = np.random.default_rng(3).integers(-4, 5, size=(21, 4)).astype(np.float32)
    r = vaq_amd.VaqMultiRefiner([0, 0], 4)
    r.set_rows(X)
    cent, q = r.fit_quantiles(bits)
    centmat = np.ascontiguousarray(cent.T)
    same_bits(centmat, lr.fit_ref("grid")[0], "the sharded fit")
    m = VaqHipMulti([0, 0], list(bits), sr.centroid_list(bits, centmat), sequential_sum=True)
    m.set_lut_quantiles(q)
    codes = m.encode_lut_from_refiner(r, return_codes=True)
    want_codes = lr.encode(X, bits, *lr.fit_ref("grid"))
    assert np.array_equal(codes, want_codes)
    m.set_option("exact_ties", 1)
    ans = m.search(queries, k)
    out = [sr.query_lut_topk(sr.row_dists(qq, bits, lr.fit_ref("grid")[0], want_codes), k) for qq in queries]
    want_l, want_d = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    assert np.array_equal(u32(ans.distances).reshape(-1, k), u32(want_d))
    assert np.array_equal(ans.labels.reshape(-1, k), want_l)
    # the single-device build gives the same, slot for slot
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(bits)
    v.fitQuantiles(X)
    v.encodeLUT(X)
    v.set_option("exact_ties", 1)
    one = v.search(queries, k)
    assert np.array_equal(one.labels, ans.labels) and np.array_equal(u32(one.distances), u32(ans.distances))
    for x in (m, r, v):
        x.close()


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/lutfit_multi_shim_test.cpp: BitVecEngineHip with setDevices({0, 0}) gives the single device's
    centroidsMat, quantiles, codebookOut and queryLUT answers"""
    import os
    import subprocess
    from vaq_amd import build
    N, D, nq = 3001, 12, 9
    rng = np.random.default_rng(12)
    bits = [int(b) for b in rng.integers(1, 9, size=D)]
    eig = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32))
    base = np.round(rng.normal(size=(N, D)) * 3).astype(np.float32)  # a coarse grid: equal distances
    queries = np.round(rng.normal(size=(nq, D)) * 3).astype(np.float32)
    data = tmp_path / "case.bin"
    with open(data, "wb") as f:
        f.write(np.array([N, D, nq], np.int32).tobytes())
        f.write(np.array(bits, np.int32).tobytes())
        f.write(eig.tobytes())
        f.write(base.tobytes())
        f.write(queries.tobytes())
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lutfit_multi_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "lutfit_multi_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lutfit_multi_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_takes_the_sharded_route(vaqlib, tmp_path):
    """examples/demo_vaqhip.cpp --lut-bits with --devices 0,0: the answers and the codebook of the run without"""
    import subprocess
    from vaq_amd import build, io
    exe = build.build_demo()
    X, bits = lr.fit_case("grid")
    k = 10
    queries = np.random.default_rng(3).integers(-4, 5, size=(21, 4)).astype(np.float32)
    io.write_vecs(str(tmp_path / "base.fvecs"), X)
    io.write_vecs(str(tmp_path / "q.fvecs"), queries)
    r = subprocess.run([exe, "--lut-bits", ",".join(map(str, bits)), "--dataset", str(tmp_path / "base.fvecs"),
                        "--queries", str(tmp_path / "q.fvecs"), "--timeseries-size", "4", "--k", str(k),
                        "--exact-ties", "1", "--devices", "0,0", "--result", str(tmp_path / "out.csv"),
                        "--save-enc", str(tmp_path / "cb.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "across 2 shards: fit" in r.stdout
    want_codes = lr.encode(X, bits, *lr.fit_ref("grid"))
    assert np.array_equal(io.load_codebook(str(tmp_path / "cb.bin")), want_codes)
    out = [sr.query_lut_topk(sr.row_dists(q, bits, lr.fit_ref("grid")[0], want_codes), k)[0] for q in queries]
    got = np.loadtxt(str(tmp_path / "out.csv"), delimiter=",", dtype=np.int64)
    assert np.array_equal(got, np.stack(out).astype(np.int64))
