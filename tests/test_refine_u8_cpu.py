"""The CPU side of byte rows in the refiners (vaqhip_[multi_]refiner_*_u8): the exported symbols, the refusals that
need no device, the bvecs reader that keeps bytes, and the byte-row forms of the exhaustive form's per-pair distance
(vaq_amd/csrc/vaq_exhaust.h) against vaq::sq_norm_eigen over the widened row."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

NEW_SYMBOLS = ("vaqhip_refiner_set_rows_u8", "vaqhip_refiner_set_rows_u8_device", "vaqhip_refiner_add_rows_u8",
               "vaqhip_multi_refiner_set_rows_u8", "vaqhip_multi_refiner_add_rows_u8", "vaqhip_refiner_elem_size",
               "vaqhip_multi_refiner_elem_size")


def test_symbols_and_version(vaqlib):
    import vaq_amd
    from vaq_amd import _lib, io
    assert vaqlib.vaqhip_version() >= 117
    for s in NEW_SYMBOLS:
        assert hasattr(vaqlib, s) and s in _lib.SYMBOLS, s
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vaqhip.h")).read()
    for s in NEW_SYMBOLS:
        assert f"int {s}(" in header, s
    for cls in (vaq_amd.VaqRefiner, vaq_amd.VaqMultiRefiner):
        for m in ("set_rows_u8", "add_rows_u8"):
            assert callable(getattr(cls, m)), (cls, m)
        assert isinstance(cls.elem_size, property)
    assert callable(io.read_bvecs_u8)


def test_refusals_touch_no_device(vaqlib):
    """EINVAL (-1) before the handle is read or a device touched: p is never dereferenced on these paths, and the codes
    are those of the float calls"""
    p = C.c_void_p(64)
    L = vaqlib
    for set_u8, set_f32, err in ((L.vaqhip_refiner_set_rows_u8, L.vaqhip_refiner_set_rows, L.vaqhip_last_error),
                                 (L.vaqhip_multi_refiner_set_rows_u8, L.vaqhip_multi_refiner_set_rows,
                                  L.vaqhip_multi_last_error)):
        for f in (set_u8, set_f32):
            assert f(None, p, 4, 0) == -1 and b"null" in err()
            assert f(p, p, -1, 0) == -1
            assert f(p, None, 4, 0) == -1
            assert f(p, p, 4, -1) == -1 and b"id_base" in err()
            assert f(p, p, 4, 0x7fffffff) == -6  # labels would pass int32: ERANGE, as the float call
    d = L.vaqhip_refiner_set_rows_u8_device
    assert d(None, p, 4, 0, None) == -1
    assert d(p, p, -1, 0, None) == -1
    assert d(p, None, 4, 0, None) == -1
    assert d(p, p, 4, -1, None) == -1
    assert d(p, p, 4, 0x7fffffff, None) == -6
    for add in (L.vaqhip_refiner_add_rows_u8, L.vaqhip_multi_refiner_add_rows_u8):
        assert add(None, p, 4) == -1
        assert add(p, p, -1) == -1
        assert add(p, None, 4) == -1
        assert add(p, p, 0) == 0  # nothing to append: the handle is not read
    assert L.vaqhip_refiner_elem_size(None) < 0 and b"null" in L.vaqhip_last_error()
    assert L.vaqhip_multi_refiner_elem_size(None) < 0 and b"null" in L.vaqhip_multi_last_error()


def test_read_bvecs_u8_round_trip(tmp_path):
    from vaq_amd import io
    rng = np.random.default_rng(3)
    X = rng.integers(0, 256, size=(37, 13), dtype=np.uint8)
    X[0, 0], X[0, 1] = 0, 255
    path = str(tmp_path / "x.bvecs")
    io.write_vecs(path, X)
    got = io.read_bvecs_u8(path)
    assert got.dtype == np.uint8 and got.flags.c_contiguous and np.array_equal(got, X)
    wide = io.read_bvecs(path)
    assert wide.dtype == np.float32 and np.array_equal(wide, got.astype(np.float32))
    assert np.array_equal(io.read_bvecs_u8(path, max_rows=5), X[:5])
    assert io.read_bvecs_u8(path, max_rows=0).shape[0] == 0


def test_byte_pair_forms_are_sq_norm_eigen(tmp_path):
    """tests/cpp/refine_u8_pair_test.cpp: xs_pair_sq_norm<.., uint8_t> and xs_widen_row + the float form ==
    sq_norm_eigen over the widened row, bit for bit, for D in {1, 7, 8, 12, 16, 40, 100, 128}, rows holding 0 and 255
    at the addresses the refiner gives them; once more under AddressSanitizer + UBSan as a stand-alone program (a load
    past a row's end or a misaligned wide load fails there)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = os.path.join(root, "tests", "cpp", "refine_u8_pair_test.cpp")
    text = open(src).read()
    assert "const int dims[] = {1, 7, 8, 12, 16, 40, 100, 128};" in text
    for extra, exe_name in ((["-O2"], "refine_u8_pair_test"),
                            (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "refine_u8_pair_asan")):
        exe = str(tmp_path / exe_name)
        subprocess.check_call([cxx, "-std=c++17", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert "refine_u8_pair_test: ok (12000 pairs)" in r.stdout
