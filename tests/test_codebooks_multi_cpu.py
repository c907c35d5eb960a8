"""The CPU side of the sharded codebook fit (vaqhip_multi_fit_codebooks*, vaqhip_multi_refiner_fit_codebooks): the C ABI
is there and refuses what it must before any device is touched, with the single fit's codes and the outputs untouched;
the Python adapters exist; and the host-only planning (vaq_amd/csrc/fit_codebooks_multi_plan.h: owners, sub-plans, the
split of the sample over the shards) holds its invariants (tests/cpp/fit_codebooks_multi_plan_test.cpp, once more under
AddressSanitizer + UBSan: host code only, its own main)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np

NEW_SYMBOLS = ("vaqhip_multi_fit_codebooks", "vaqhip_multi_fit_codebooks_u8", "vaqhip_multi_refiner_fit_codebooks",
               "vaqhip_multi_last_fit_codebooks_timing")
NO_SUCH_DEVICES = [977, 978, 979]  # never touched: every refusal below is decided first
SENTINEL = 7.25


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_symbols_and_adapters(vaqlib):
    import vaq_amd
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 121
    for s in NEW_SYMBOLS:
        assert hasattr(vaqlib, s) and s in _lib.SYMBOLS, s
    assert hasattr(vaq_amd.VaqMultiRefiner, "fit_codebooks")
    assert callable(vaq_amd.last_multi_fit_codebooks_timing)
    for fn in (vaq_amd.fit_codebooks, vaq_amd.fit_codebooks_u8):
        params = inspect.signature(fn).parameters
        assert "devices" in params and "device" in params


def test_refusals_touch_no_device(vaqlib):
    """The single fit's refusals with its codes, then the device list's; nothing is written."""
    X = np.zeros((8, 4), np.float32)
    cent = np.full(64, SENTINEL, np.float32)
    iters = np.full(2, -9, np.int32)
    nan = np.full(2, -9, np.int32)

    def fit(n, D, M, bits, x=X, c=cent, devs=NO_SUCH_DEVICES, G=None, max_iter=25, fn=vaqlib.vaqhip_multi_fit_codebooks):
        b = (C.c_int * max(len(bits), 1))(*bits) if bits is not None else None
        d = (C.c_int * len(devs))(*devs) if devs is not None else None
        G = (len(devs) if devs is not None else 1) if G is None else G
        return fn(G, d, _p(x), n, D, M, b, None, max_iter, _p(c), _p(iters), _p(nan))

    err = vaqlib.vaqhip_multi_last_error
    assert fit(8, 4, 2, [0, 2]) == -1 and b"bits[0]=0" in err()
    assert fit(8, 4, 2, [2, 16]) == -1 and b"bits[1]=16" in err()
    assert fit(8, 4, 2, [2, 4]) == -1 and b"16 centres from 8 rows" in err()
    assert fit(0, 4, 2, [2, 2]) == -1
    assert fit(1 << 31, 4, 2, [2, 2]) == -1 and b"randomPermutation" in err()
    assert fit(8, 4, 3, [2, 2, 2]) == -1 and b"subspaces of equal length" in err()
    assert fit(8, 4, 0, []) == -1
    assert fit(8, 4, 2, [2, 2], max_iter=0) == -1 and b"max_iter=0" in err()
    assert fit(8, 129, 129, [1] * 129) == -2      # EUNSUPPORTED, as the single fit
    assert fit(8, 4100, 2, [2, 2]) == -2
    assert fit(8, 4, 2, None) == -1
    assert fit(8, 4, 2, [2, 2], x=None) == -1
    assert fit(8, 4, 2, [2, 2], c=None) == -1
    assert fit(8, 4, 2, [2, 2], devs=None) == -1
    assert fit(8, 4, 2, [2, 2], G=0) == -1 and b"n_devices=0" in err()
    assert fit(8, 4, 2, [2, 2], devs=[977] * 17) == -1 and b"n_devices=17" in err()
    assert fit(8, 4, 2, [2, 2], G=-3) == -1
    X8 = np.zeros((8, 4), np.uint8)
    assert fit(8, 4, 2, [2, 4], x=X8, fn=vaqlib.vaqhip_multi_fit_codebooks_u8) == -1 and b"16 centres from 8 rows" in err()
    assert fit(8, 4, 2, [2, 2], x=X8, G=17, fn=vaqlib.vaqhip_multi_fit_codebooks_u8) == -1 and b"n_devices=17" in err()
    assert np.all(cent == SENTINEL) and np.all(iters == -9) and np.all(nan == -9)


def test_setup_and_teardown_on_devices_that_do_not_exist(vaqlib):
    """Valid arguments, so the call-owned run (vaq_amd/csrc/vaqhip_shard_run.h) starts its workers, fails in the first
    step of every shard's setup and is taken down with no shard opened; twice, so that a teardown which leaves the pool
    or the thread's state broken shows.  The same on a machine with GPUs: ordinal 977 exists on none."""
    X = np.zeros((8, 4), np.float32)
    bits = (C.c_int * 4)(3, 3, 3, 3)
    devs = (C.c_int * 2)(977, 978)
    for _ in range(2):
        cent = np.full(4 * 8, SENTINEL, np.float32)
        iters = np.full(4, -9, np.int32)
        nan = np.full(4, -9, np.int32)
        rc = vaqlib.vaqhip_multi_fit_codebooks(2, devs, _p(X), 8, 4, 4, bits, None, 5, _p(cent), _p(iters), _p(nan))
        assert rc == -3  # ENODEVICE
        assert vaqlib.vaqhip_multi_last_error() == b"shard 0 (device 977): hipSetDevice failed (no CPU path)"
        assert np.all(cent == SENTINEL) and np.all(iters == -9) and np.all(nan == -9)


def test_refiner_form_refuses_null(vaqlib):
    cent = np.full(64, SENTINEL, np.float32)
    bits = (C.c_int * 2)(2, 2)
    assert vaqlib.vaqhip_multi_refiner_fit_codebooks(None, 2, bits, None, 25, _p(cent), None, None) == -1
    assert b"refiner is null" in vaqlib.vaqhip_multi_last_error()
    assert np.all(cent == SENTINEL)
    assert vaqlib.vaqhip_multi_last_fit_codebooks_timing(None) == -1


def test_timing_struct_layout(vaqlib):
    from vaq_amd import _lib
    t = _lib.MultiFitCodebooksTiming()
    assert [f for f, _ in t._fields_] == ["total_ms", "columns_ms", "copy_ms", "place_ms", "assign_ms", "accumulate_ms",
                                          "update_ms", "iterations", "subspaces", "dims", "rows", "sample_rows",
                                          "n_devices", "owner_subspaces"]
    assert C.sizeof(t) == 7 * 4 + 3 * 4 + 2 * 8 + 4 + 16 * 4 + 4  # (one int of tail padding: the struct holds int64_t)
    assert vaqlib.vaqhip_multi_last_fit_codebooks_timing(C.byref(t)) == 0


def test_planning_header(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    for extra, name in ((["-O2"], "fit_codebooks_multi_plan_test"),
                        (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "fit_codebooks_multi_plan_asan")):
        exe = str(tmp_path / name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [os.path.join(root, "tests", "cpp", "fit_codebooks_multi_plan_test.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert "fit_codebooks_multi_plan_test: ok" in r.stdout
