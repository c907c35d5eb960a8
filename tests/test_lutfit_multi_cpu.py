"""The CPU side of building a queryLUT index across the shards of a multi-device index: the C ABI is there and
refuses what it must before any device is touched, the Python adapters exist, and the host-only planning of the
sharded fit (vaq_amd/csrc/lutfit_multi_plan.h: owners, rounds, offsets) holds its invariants
(tests/cpp/lutfit_multi_plan_test.cpp, once more under AddressSanitizer + UBSan: host code only, its own main)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

NEW_SYMBOLS = ("vaqhip_multi_lut_fit_quantiles", "vaqhip_multi_refiner_lut_fit_quantiles",
               "vaqhip_multi_last_lut_fit_timing", "vaqhip_multi_set_lut_quantiles", "vaqhip_multi_encode_lut_set_codes",
               "vaqhip_multi_encode_lut_add_codes", "vaqhip_multi_encode_lut_from_refiner")
NO_SUCH_DEVICES = [977, 978, 979]  # never touched: every refusal below is decided first
SENTINEL = 7.25


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_symbols_and_version(vaqlib):
    import vaq_amd
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 116
    for s in NEW_SYMBOLS:
        assert hasattr(vaqlib, s) and s in _lib.SYMBOLS, s
    for m in ("set_lut_quantiles", "encode_lut", "encode_lut_add", "encode_lut_from_refiner"):
        assert hasattr(vaq_amd.VaqHipMulti, m), m
    assert hasattr(vaq_amd.VaqMultiRefiner, "fit_quantiles")
    assert callable(vaq_amd.lut_fit_quantiles_multi)
    import inspect
    assert "devices" in inspect.signature(vaq_amd.VaqHip.fitQuantiles).parameters


def test_fit_refusals_touch_no_device(vaqlib):
    X = np.zeros((4, 2), np.float32)
    cent = np.full((2, 256), SENTINEL, np.float32)
    q = np.full((2, 257), SENTINEL, np.float32)

    def fit(n, D, bits, x=X, c=cent, qq=q, devs=NO_SUCH_DEVICES, G=None):
        b = (C.c_int * max(len(bits), 1))(*bits) if bits is not None else None
        d = (C.c_int * len(devs))(*devs) if devs is not None else None
        G = (len(devs) if devs is not None else 1) if G is None else G
        return vaqlib.vaqhip_multi_lut_fit_quantiles(G, d, _p(x), n, D, b, None, _p(c), _p(qq))

    err = vaqlib.vaqhip_multi_last_error
    assert fit(4, 2, [0, 3]) == -1 and b"bits[0]=0" in err()
    assert fit(4, 2, [3, 9]) == -1 and b"bits[1]=9" in err()
    assert fit(0, 2, [3, 3]) == -1
    assert fit(-5, 2, [3, 3]) == -1
    assert fit(1 << 31, 2, [3, 3]) == -1 and b"counts a bucket in an int" in err()
    assert fit(4, 0, []) == -1
    assert fit(4, 4097, [3] * 4097) == -2   # EUNSUPPORTED, as the single fit
    assert fit(4, 2, None) == -1
    assert fit(4, 2, [3, 3], x=None) == -1
    assert fit(4, 2, [3, 3], c=None) == -1
    assert fit(4, 2, [3, 3], qq=None) == -1
    assert fit(4, 2, [3, 3], devs=None) == -1
    assert fit(4, 2, [3, 3], G=0) == -1 and b"n_devices=0" in err()
    assert fit(4, 2, [3, 3], devs=[977] * 17) == -1 and b"n_devices=17" in err()
    assert fit(4, 2, [3, 3], G=-3) == -1
    assert np.all(cent == SENTINEL) and np.all(q == SENTINEL)


def test_setup_and_teardown_on_devices_that_do_not_exist(vaqlib):
    """Valid arguments, so the call-owned run (vaq_amd/csrc/vaqhip_shard_run.h) starts its workers, fails in the first
    step of every shard's setup and is taken down with no shard opened; twice, so that a teardown which leaves the pool
    or the thread's state broken shows.  The same on a machine with GPUs: ordinal 977 exists on none."""
    X = np.zeros((8, 4), np.float32)
    bits = (C.c_int * 4)(3, 3, 3, 3)
    devs = (C.c_int * 2)(977, 978)
    for _ in range(2):
        cent = np.full((4, 256), SENTINEL, np.float32)
        q = np.full((4, 257), SENTINEL, np.float32)
        assert vaqlib.vaqhip_multi_lut_fit_quantiles(2, devs, _p(X), 8, 4, bits, None, _p(cent), _p(q)) == -3  # ENODEVICE
        assert vaqlib.vaqhip_multi_last_error() == b"shard 0 (device 977): hipSetDevice failed (no CPU path)"
        assert np.all(cent == SENTINEL) and np.all(q == SENTINEL)


def test_refiner_form_and_setters_refuse_null(vaqlib):
    cent = np.full((2, 256), SENTINEL, np.float32)
    q = np.full((2, 257), SENTINEL, np.float32)
    bits = (C.c_int * 2)(3, 3)
    assert vaqlib.vaqhip_multi_refiner_lut_fit_quantiles(None, bits, None, _p(cent), _p(q)) == -1
    assert b"refiner is null" in vaqlib.vaqhip_multi_last_error()
    assert np.all(cent == SENTINEL) and np.all(q == SENTINEL)
    assert vaqlib.vaqhip_multi_last_lut_fit_timing(None) == -1
    assert vaqlib.vaqhip_multi_set_lut_quantiles(None, _p(q)) == -1
    X = np.zeros((4, 2), np.float32)
    assert vaqlib.vaqhip_multi_encode_lut_set_codes(None, _p(X), 4, 1, 0, None) == -1
    assert vaqlib.vaqhip_multi_encode_lut_add_codes(None, _p(X), 4, 1, None) == -1
    assert vaqlib.vaqhip_multi_encode_lut_from_refiner(None, None, None) == -1


def test_timing_struct_layout(vaqlib):
    from vaq_amd import _lib
    t = _lib.MultiLutFitTiming()
    assert [f for f, _ in t._fields_] == ["total_ms", "columns_ms", "copy_ms", "sort_ms", "quantile_ms", "means_ms",
                                          "rows", "dims", "n_devices"]
    assert vaqlib.vaqhip_multi_last_lut_fit_timing(C.byref(t)) == 0
    assert t.rows == 0 and t.n_devices == 0  # no sharded fit on this thread yet


def test_planning_header(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    for extra, name in ((["-O2"], "lutfit_multi_plan_test"),
                        (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "lutfit_multi_plan_asan")):
        exe = str(tmp_path / name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [os.path.join(root, "tests", "cpp", "lutfit_multi_plan_test.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert "lutfit_multi_plan_test: ok" in r.stdout
