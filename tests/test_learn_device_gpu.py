"""learnQuantization's device forms on the GPU: every form against vaqhip_learn_quantization (the host form) on the
same rows, bit for bit -- return code, offsets, scale, the chosen alpha -- and the seven losses against the NumPy
restatement (tests/learn_ref.py), bit for bit.

Shapes: the mixed code widths are [4, 4, 3, 2, 1, 4, 4, 4]: M must be a multiple of 4 for FAST (the grouped row sum),
and the narrow subspaces' table rows are zero-padded to 16."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fast_ref as fr
import learn_ref as lr
from helpers import make_case

pytestmark = pytest.mark.gpu

MIXED = [4, 4, 3, 2, 1, 4, 4, 4]
UNTOUCHED = np.float32(7.0)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def fast_index(c):
    import vaq_amd
    v = vaq_amd.VaqHipFast(device=0)
    v.parseMethodString(f"VAQ{sum(c['bits'])}m{c['M']}min1max{max(c['bits'])}var1,FAST")
    v.mBitsAlloc = c["bits"]
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    v._ensure_codes()
    return v


def ratio_for(n, sample):
    """a ratio with int(float32(ratio) * float32(n)) == sample"""
    r = np.float32(1.0) if sample == n else np.float32((sample + 0.5) / n)
    assert int(r * np.float32(n)) == sample
    return float(r)


def raw(fn, h, *args):
    """(code, offsets, scale) of one learn call; the outputs start as UNTOUCHED"""
    from vaq_amd import _lib
    inf = _lib.Info()
    assert _lib.load().vaqhip_index_info(h, C.byref(inf)) == 0
    off = np.full(inf.M, UNTOUCHED, np.float32)
    sc = np.full(inf.M, UNTOUCHED, np.float32)
    return fn(h, *args, p(off), p(sc)), off, sc


def timing(h):
    from vaq_amd import _lib
    t = _lib.LearnTiming()
    assert _lib.load().vaqhip_last_learn_timing(h, C.byref(t)) == 0
    return t


def same(a, b, what):
    assert a[0] == b[0], f"{what}: code {a[0]} against the host form's {b[0]}"
    if b[0] == 0:
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), what
    else:
        assert np.all(a[1] == UNTOUCHED) and np.all(a[2] == UNTOUCHED), f"{what}: outputs written by a failed call"


def rows_for(seed, n, D):
    rng = np.random.default_rng(seed)
    Xb = rng.integers(0, 256, size=(n, D), dtype=np.uint8)
    Xc = (rng.normal(size=(n, D)) * 30).astype(np.float32)
    return Xb, Xc


@pytest.mark.parametrize("n", [2, 10, 257, 4001])
@pytest.mark.parametrize("D,bits", [(16, MIXED), (32, [4] * 8), (32, MIXED)])
def test_every_form_equals_the_host_form(vaqlib, D, bits, n):
    import torch
    import vaq_amd
    L = vaqlib
    c = make_case(300 + n + D, D, bits, 50, 3)
    v = fast_index(c)
    h = v._h
    Xb, Xc = rows_for(n, n, D)
    Xbf = Xb.astype(np.float32)
    d_b, d_bf, d_c = torch.from_numpy(Xb).cuda(), torch.from_numpy(Xbf).cuda(), torch.from_numpy(Xc).cuda()
    torch.cuda.synchronize()
    dp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rb = vaq_amd.VaqRefiner(D, device=0)
    cut = n // 3
    rb.set_rows_u8(Xb[:cut] if cut else Xb, id_base=5)
    if cut:
        rb.add_rows_u8(Xb[cut:])
    rc_ = vaq_amd.VaqRefiner(D, device=0)
    rc_.set_rows(Xc)
    for sample in sorted({1, min(2, n), n - 1, n} - {0}):
        ratio = C.c_float(ratio_for(n, sample))
        rows = fr.sample_rows(n, ratio.value)
        assert rows.shape[0] == sample
        for projected in (0, 1):
            what = f"D={D} n={n} sample={sample} projected={projected}"
            host_b = raw(L.vaqhip_learn_quantization, h, p(Xbf), n, projected, ratio)
            host_c = raw(L.vaqhip_learn_quantization, h, p(Xc), n, projected, ratio)
            got = raw(L.vaqhip_learn_quantization_u8, h, p(Xb), n, projected, ratio)
            same(got, host_b, what + " _u8")
            got = raw(L.vaqhip_learn_quantization_u8_device, h, dp(d_b), n, projected, ratio)
            same(got, host_b, what + " _u8_device")
            got = raw(L.vaqhip_learn_quantization_device, h, dp(d_bf), n, projected, ratio)
            same(got, host_b, what + " _device, byte-valued")
            got = raw(L.vaqhip_learn_quantization_device, h, dp(d_c), n, projected, ratio)
            same(got, host_c, what + " _device")
            # the losses, the chosen alpha and the checker, on the continuous rows
            t = timing(h)
            assert t.sample_rows == sample and t.column_groups == 1
            eo, es, ea, eloss, scales = lr.learn(v.build_lut(Xc[rows], projected=bool(projected)))
            assert t.chosen_alpha == ea, what
            assert np.array_equal(np.array(list(t.loss)), eloss, equal_nan=True), what
            if got[0] == 0:
                assert np.array_equal(got[1], eo) and np.array_equal(got[2], es), what
            # (fast_ref casts a negative float to uint8 directly, which is the platform's choice: it is asked where no
            #  alpha's scale is negative)
            if got[0] == 0 and np.all(scales > 0):
                fo, fs, fa = fr.learn_from_luts(fr.stack_luts(v.build_lut(Xc[rows], projected=bool(projected))))
                assert fa == ea and np.array_equal(got[1], fo) and np.array_equal(got[2], fs), what
        # the refiners hold raw rows
        host_b = raw(L.vaqhip_learn_quantization, h, p(Xbf), n, 0, ratio)
        host_c = raw(L.vaqhip_learn_quantization, h, p(Xc), n, 0, ratio)
        same(raw(L.vaqhip_learn_quantization_from_refiner, h, rb._h, ratio), host_b, f"byte refiner n={n} sample={sample}")
        same(raw(L.vaqhip_learn_quantization_from_refiner, h, rc_._h, ratio), host_c, f"float refiner n={n} sample={sample}")
    rb.close()
    rc_.close()
    v.close()


@pytest.mark.parametrize("bits", [MIXED, [4] * 8])
def test_column_groups_do_not_change_the_result(vaqlib, bits):
    L = vaqlib
    n, D, sample = 4001, 32, 400
    c = make_case(77, D, bits, 50, 3)
    v = fast_index(c)
    Xb, Xc = rows_for(9, n, D)
    ratio = C.c_float(ratio_for(n, sample))
    host = raw(L.vaqhip_learn_quantization, v._h, p(Xc), n, 0, ratio)
    assert host[0] == 0
    seen = []
    try:
        for mc in (1, 3, 8):
            assert L.vaqhip_learn_set_workspace(sample * 16 * 4 * (mc + 4)) == 0
            got = raw(L.vaqhip_learn_quantization_u8, v._h, p(Xb), n, 0, ratio)  # (another result between)
            assert got[0] == 0
            got = raw(L.vaqhip_learn_quantization_device, v._h, C.c_void_p(_cuda(Xc).data_ptr()), n, 0, ratio)
            same(got, host, f"Mc={mc}")
            t = timing(v._h)
            assert t.column_groups == -(-8 // mc)
            seen.append((t.chosen_alpha, list(t.loss)))
    finally:
        assert L.vaqhip_learn_set_workspace(0) == 0
    assert seen[0] == seen[1] == seen[2]
    v.close()


_keep = []


def _cuda(a):
    import torch
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    _keep[:] = [t]
    return t


def _last_shard_case(G):
    """(n, sample) whose sampled rows all lie in the last of G shards (the cut of the multi refiner)"""
    for n in range(G + 1, 200):
        per = -(-n // G)
        lo = per * (G - 1)
        for sample in (2, 1):
            if lo < n and sample <= n and np.all(fr.sample_rows(n, ratio_for(n, sample)) >= lo):
                return n, sample
    raise AssertionError("no such case")


@pytest.mark.parametrize("devices", [[0, 0, 0], [0]])
def test_multi_refiner_forms(vaqlib, devices):
    import vaq_amd
    from vaq_amd.index import VaqHipMulti, VaqMultiRefiner
    L = vaqlib
    D, G = 16, len(devices)
    c = make_case(41, D, MIXED, 50, 5)
    v = fast_index(c)
    m = VaqHipMulti(devices, c["bits"], c["cents"], c["eig"])
    m.set_codes(c["codes"])
    r = VaqMultiRefiner(devices, D)
    n_last, s_last = _last_shard_case(3)
    for n, sample, u8 in [(2, 1, False), (2, 2, True), (10, 9, True), (257, 100, False), (4001, 400, True),
                          (n_last, s_last, False)]:
        Xb, Xc = rows_for(1000 + n, n, D)
        ratio = ratio_for(n, sample)
        what = f"devices={devices} n={n} sample={sample} u8={u8}"
        if u8:
            r.set_rows_u8(Xb, id_base=11)
            host = raw(L.vaqhip_learn_quantization, v._h, p(Xb.astype(np.float32)), n, 0, C.c_float(ratio))
        else:
            r.set_rows(Xc, id_base=3)
            host = raw(L.vaqhip_learn_quantization, v._h, p(Xc), n, 0, C.c_float(ratio))
        if host[0] != 0:
            with pytest.raises(vaq_amd.VaqHipError) as e:
                m.learn_quantization_from_refiner(r, ratio)
            assert e.value.code == host[0], what
            continue
        off, sc = m.learn_quantization_from_refiner(r, ratio)
        assert np.array_equal(off.view(np.uint32), host[1].view(np.uint32)), what
        assert np.array_equal(sc.view(np.uint32), host[2].view(np.uint32)), what
        want = v.buildSmallLUT(c["X"])
        for g in range(G):
            got = np.empty_like(want)
            assert L.vaqhip_build_small_lut(C.c_void_p(m.shard(g)), p(c["X"]), c["X"].shape[0], 0, p(got)) == 0
            assert np.array_equal(got, want), what + f" shard {g}"
        if u8:  # the host byte form on the multi index
            off, sc = m.learn_quantization_u8(Xb, ratio)
            assert np.array_equal(off.view(np.uint32), host[1].view(np.uint32)), what
            assert np.array_equal(sc.view(np.uint32), host[2].view(np.uint32)), what
    r.close()
    m.close()
    v.close()


def test_end_to_end_from_a_byte_refiner(vaqlib):
    """learnt and encoded from bytes, searched with FAST: the slots of the index built from the host float matrix"""
    import vaq_amd
    n, D, nq, k = 2000, 32, 33, 10
    c = make_case(90, D, [4] * 8, 10, nq)
    Xb, _ = rows_for(5, n, D)
    a = fast_index(c)
    a.learnQuantization(Xb.astype(np.float32), 0.1)
    a.encode(Xb.astype(np.float32), projected=False)
    want = a.search(c["X"], k)
    b = fast_index(c)
    r = vaq_amd.VaqRefiner(D, device=0)
    r.set_rows_u8(Xb)
    b.learnQuantizationFromRefiner(r, 0.1)
    assert np.array_equal(b.mOffsets, a.mOffsets) and np.array_equal(b.mScale, a.mScale)
    assert b.last_learn_timing()["sample_rows"] == 200
    b.encode_u8(Xb, projected=False)
    got = b.search(c["X"], k)
    assert np.array_equal(got.labels, want.labels) and np.array_equal(got.distances, want.distances)
    assert np.all(want.labels.reshape(nq, k) >= 0)
    r.close()
    a.close()
    b.close()


def test_degenerate_rows(vaqlib):
    L = vaqlib
    n, D, sample = 257, 16, 60
    c = make_case(55, D, [4] * 8, 50, 4)
    v = fast_index(c)
    h = v._h
    _, Xc = rows_for(3, n, D)
    ratio = C.c_float(ratio_for(n, sample))
    rows = fr.sample_rows(n, ratio.value)
    good = raw(L.vaqhip_learn_quantization_device, h, C.c_void_p(_cuda(Xc).data_ptr()), n, 0, ratio)
    assert good[0] == 0
    v.mOffsets, v.mScale = good[1], good[2]
    before = v.buildSmallLUT(c["X"])
    # all rows identical: ceil = 0 in every column
    Xi = np.ascontiguousarray(np.broadcast_to(Xc[0], (n, D)))
    host = raw(L.vaqhip_learn_quantization, h, p(Xi), n, 0, ratio)
    # (the host form has set nothing either when it failed; when it succeeded the test below compares the values)
    got = raw(L.vaqhip_learn_quantization_device, h, C.c_void_p(_cuda(Xi).data_ptr()), n, 0, ratio)
    same(got, host, "identical rows")
    if host[0] != 0:
        assert np.array_equal(v.buildSmallLUT(c["X"]), before)
    # a NaN in a sampled row: refused, nothing written, the quantisation stays
    assert raw(L.vaqhip_learn_quantization_device, h, C.c_void_p(_cuda(Xc).data_ptr()), n, 0, ratio)[0] == 0
    Xn = Xc.copy()
    Xn[rows[sample // 2], 3] = np.nan
    got = raw(L.vaqhip_learn_quantization_device, h, C.c_void_p(_cuda(Xn).data_ptr()), n, 0, ratio)
    assert got[0] == -1 and b"NaN" in L.vaqhip_last_error()
    assert np.all(got[1] == UNTOUCHED) and np.all(got[2] == UNTOUCHED)
    assert np.array_equal(v.buildSmallLUT(c["X"]), before)
    # a NaN in a row the sample leaves out plays no part
    Xu = Xc.copy()
    Xu[np.setdiff1d(np.arange(n), rows)[0], 3] = np.nan
    got = raw(L.vaqhip_learn_quantization_device, h, C.c_void_p(_cuda(Xu).data_ptr()), n, 0, ratio)
    same(got, good, "NaN in an unsampled row")
    v.close()


def test_refusals_match_the_float_form(vaqlib):
    import vaq_amd
    L = vaqlib
    D = 16
    c = make_case(56, D, [4] * 8, 50, 4)
    v = fast_index(c)
    h = v._h
    Xb = np.zeros((20, D), np.uint8)
    Xf = np.zeros((20, D), np.float32)
    d = _cuda(Xf)
    dp = C.c_void_p(d.data_ptr())
    half = C.c_float(0.5)
    new = [(L.vaqhip_learn_quantization_u8, p(Xb)), (L.vaqhip_learn_quantization_device, dp),
           (L.vaqhip_learn_quantization_u8_device, dp)]
    for args, code in [((None, 20, 0, half), -1), ((p(Xf), 0, 0, half), -1), ((p(Xf), -3, 0, half), -1),
                       ((p(Xf), 1 << 31, 0, half), -6), ((p(Xf), 20, 0, C.c_float(0.01)), -1)]:
        assert raw(L.vaqhip_learn_quantization, h, *args)[0] == code
        for fn, x in new:
            a = (x if args[0] is not None else None,) + args[1:]
            got = raw(fn, h, *a)
            assert got[0] == code and np.all(got[1] == UNTOUCHED), (fn.__name__, args[1:])
    for fn, x in new:  # a ratio above 1: the host form reads past its permutation, the new forms refuse
        assert raw(fn, h, x, 20, 0, C.c_float(1.5))[0] == -1
    # an index that cannot hold FAST codes
    w = make_case(57, D, [8] * 8, 10, 1)
    hv = vaq_amd.VaqHip(device=0)
    hv.mBitsAlloc, hv.mCentroidsPerSubs, hv.mEigenVectors, hv.mCodebook = w["bits"], w["cents"], None, w["codes"]
    hv._ensure_codes()
    assert raw(L.vaqhip_learn_quantization, hv._h, p(Xf), 20, 0, half)[0] == -2
    for fn, x in new:
        assert raw(fn, hv._h, x, 20, 0, half)[0] == -2
    # refiners: no rows, another D
    r = vaq_amd.VaqRefiner(D, device=0)
    assert raw(L.vaqhip_learn_quantization_from_refiner, h, r._h, half)[0] == -7
    r.set_rows(Xf)
    assert raw(L.vaqhip_learn_quantization_from_refiner, hv._h, r._h, half)[0] == -2
    assert raw(L.vaqhip_learn_quantization_from_refiner, h, None, half)[0] == -1
    r2 = vaq_amd.VaqRefiner(D * 2, device=0)
    r2.set_rows(np.zeros((20, 2 * D), np.float32))
    assert raw(L.vaqhip_learn_quantization_from_refiner, h, r2._h, half)[0] == -1
    for x in (r, r2, hv, v):
        x.close()


def test_python_wrappers(vaqlib):
    """the VaqHipFast / VaqHipMulti methods themselves: mOffsets / mScale of learnQuantization() on the same rows, and a
    FAST search served from them without another push"""
    import torch
    import vaq_amd
    from vaq_amd.index import VaqHipMulti
    n, D, ratio = 1000, 32, 0.25
    c = make_case(91, D, MIXED, 300, 7)
    Xb, Xc = rows_for(6, n, D)
    a = fast_index(c)

    def want(X, projected):
        a.learnQuantization(X, ratio, projected=projected)
        return a.mOffsets.copy(), a.mScale.copy(), a.search(c["X"], 10)

    def check(v, w, what):
        assert np.array_equal(v.mOffsets.view(np.uint32), w[0].view(np.uint32)), what
        assert np.array_equal(v.mScale.view(np.uint32), w[1].view(np.uint32)), what
        got = v.search(c["X"], 10)
        assert np.array_equal(got.labels, w[2].labels) and np.array_equal(got.distances, w[2].distances), what
        assert v.last_learn_timing()["sample_rows"] == 250

    for projected in (False, True):
        wb, wc = want(Xb.astype(np.float32), projected), want(Xc, projected)
        v = fast_index(c)
        v.learnQuantization_u8(Xb, ratio, projected=projected)
        check(v, wb, f"learnQuantization_u8 projected={projected}")
        d = torch.from_numpy(Xc).cuda() * 1.0  # (produced on torch's stream: the wrapper waits for it)
        v.learnQuantization_device(d, ratio, projected=projected)
        check(v, wc, f"learnQuantization_device projected={projected}")
        v.learnQuantization_u8_device(torch.from_numpy(Xb).cuda(), ratio, projected=projected)
        check(v, wb, f"learnQuantization_u8_device projected={projected}")
        v.close()
    wb = want(Xb.astype(np.float32), False)
    v = fast_index(c)
    r = vaq_amd.VaqRefiner(D, device=0)
    r.set_rows_u8(Xb)
    v.learnQuantizationFromRefiner(r, ratio)
    check(v, wb, "learnQuantizationFromRefiner")
    m = VaqHipMulti([0, 0], c["bits"], c["cents"], c["eig"])
    off, sc = m.learn_quantization_u8(Xb, ratio)
    assert np.array_equal(off.view(np.uint32), wb[0].view(np.uint32)) and np.array_equal(sc.view(np.uint32), wb[1].view(np.uint32))
    with pytest.raises(vaq_amd.VaqHipError):
        m.learn_quantization_u8(Xb.astype(np.float32), ratio)
    for x in (m, r, v, a):
        x.close()


def _write_case(path, c, base, queries):
    with open(path, "wb") as f:
        f.write(np.array([base.shape[0], c["M"], c["L"], 4, queries.shape[0]], np.int32).tobytes())
        for cent in c["cents"]:
            f.write(np.ascontiguousarray(cent, np.float32).tobytes())
        f.write(np.ascontiguousarray(c["eig"], np.float32).tobytes())
        f.write(base.tobytes())
        f.write(np.ascontiguousarray(queries, np.float32).tobytes())


def test_cpp_shim(vaqlib, tmp_path):
    """tests/cpp/learn_shim_test.cpp: VaqHipFast::learnQuantization(RowMatrix<uint8_t>) and learnQuantizationRefineDataset
    on one device and after setDevices(), against the float overload"""
    from vaq_amd import build
    N, M, L, nq = 2000, 8, 4, 9
    D = M * L
    c = make_case(737, D, [4] * M, 0, nq, rotate=True, scale=60.0)
    c["cents"] = [cc + 100 for cc in c["cents"]]
    base, _ = rows_for(21, N, D)
    data = tmp_path / "case.bin"
    _write_case(data, c, base, c["X"] + 128)
    lib = build.build_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "learn_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "learn_shim_test.cpp"), "-o", exe,
                           "-L" + os.path.dirname(lib), "-lvaqhip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "learn_shim ok" in r.stdout, r.stdout + r.stderr


def test_demo_learns_from_bytes_and_from_the_resident_rows(vaqlib, tmp_path):
    """demo_vaqhip with a FAST method: --file-format-ori bvecs learns from the bytes, --refine-resident from the rows on
    the device(s); the answers are those of the fvecs run, which learns from the host float matrix"""
    from vaq_amd import build, io
    exe = build.build_demo()
    N, M, L, nq, k = 1000, 8, 4, 9, 10
    D = M * L
    c = make_case(738, D, [4] * M, 0, nq, rotate=True, scale=60.0)
    X, _ = rows_for(22, N, D)
    Xq = np.random.default_rng(11).integers(0, 256, size=(nq, D), dtype=np.uint8)
    for name, arr in (("base", X), ("q", Xq)):
        io.write_vecs(str(tmp_path / f"{name}.bvecs"), arr)
        io.write_vecs(str(tmp_path / f"{name}.fvecs"), arr.astype(np.float32))
    io.save_centroids([np.ascontiguousarray(cc + 100, np.float32) for cc in c["cents"]], str(tmp_path / "cent.bin"))
    np.ascontiguousarray(c["eig"], np.float32).tofile(str(tmp_path / "eig.f32"))

    import shutil
    shutil.copy(str(tmp_path / "base.fvecs"), str(tmp_path / "raw.fvecs"))  # the same rows under another name
    runs = []

    def run(fmt, extra):
        tag = f"run{len(runs)}"
        runs.append(tag)
        r = subprocess.run([exe, "--encode", "--centroids", str(tmp_path / "cent.bin"), "--method", f"VAQ{4 * M}m{M}min4max4var1,FAST",
                            "--eigen", str(tmp_path / "eig.f32"), "--dataset", str(tmp_path / f"base.{fmt}"),
                            "--queries", str(tmp_path / f"q.{fmt}"), "--file-format-ori", fmt, "--learn-ratio", "0.2",
                            "--timeseries-size", str(D), "--k", str(k), "--result", str(tmp_path / f"{tag}.csv")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        learnt = [ln for ln in r.stdout.splitlines() if "Learn Quantization time" in ln]
        assert len(learnt) == 1, r.stdout
        return learnt[0], np.loadtxt(str(tmp_path / f"{tag}.csv"), delimiter=",", dtype=np.int64)

    line, want = run("fvecs", [])
    assert "(from" not in line  # the host float matrix, as the reference
    line, got = run("bvecs", [])
    assert "from the byte rows of the bvecs file" in line
    assert np.array_equal(got, want)
    resident = ["--refine-resident", "--refine", "20"]
    for dev in ([], ["--devices", "0,0"]):
        # --dataset-refine names another file: the quantisation is learnt from the host matrix, the refine is the same
        line, want = run("fvecs", resident + ["--dataset-refine", str(tmp_path / "raw.fvecs")] + dev)
        assert "(from" not in line
        for fmt in ("fvecs", "bvecs"):
            line, got = run(fmt, resident + dev)
            assert "(from the resident rows)" in line, line
            assert np.array_equal(got, want), (fmt, dev)
