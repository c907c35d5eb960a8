"""The CPU side of the multi-device refiner (vaqhip_multi_refiner_*): the cut of the rows and the way from a label to
the shard that owns it (vaq_amd/csrc/refine_owner.h, compiled by the host and by the select kernel alike) as a
stand-alone program, and the new entry points of the C ABI without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

NEW_SYMBOLS = ("vaqhip_multi_refiner_create", "vaqhip_multi_refiner_destroy", "vaqhip_multi_refiner_set_rows",
               "vaqhip_multi_refiner_add_rows", "vaqhip_multi_refiner_set_option", "vaqhip_multi_refiner_refine",
               "vaqhip_multi_refiner_refine_device", "vaqhip_multi_search_refine", "vaqhip_multi_search_refine_device",
               "vaqhip_multi_refiner_get_info")


@pytest.mark.parametrize("flags,exe_name", [
    (["-O2"], "refine_owner_test"),
    (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "refine_owner_asan")])
def test_label_to_shard(tmp_path, flags, exe_name):
    """tests/cpp/refine_owner_test.cpp: every label of [id_base - 2, id_base + N + 2) for N in {0, 1, 5, 300, 3000} x
    G in {1, 2, 3, 8, 16} against a linear scan, a last shard grown by appends, id_base near 2^31; once optimised and
    once under AddressSanitizer + UBSan (a stand-alone program: nothing is loaded into python)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / exe_name)
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-I" + os.path.join(root, "vaq_amd", "csrc")] + flags +
                          [os.path.join(root, "tests", "cpp", "refine_owner_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "refine_owner_test: ok" in r.stdout


def test_abi_has_the_multi_refiner(vaqlib):
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 112
    for s in NEW_SYMBOLS:
        assert hasattr(vaqlib, s) and s in _lib.SYMBOLS, s
    import vaq_amd
    assert vaq_amd.VaqMultiRefiner and hasattr(vaq_amd.VaqHipMulti, "search_refine")


def test_create_validates_and_needs_a_gpu(vaqlib):
    h = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert vaqlib.vaqhip_multi_refiner_create(None, 8, 2, devs) == -1
    assert vaqlib.vaqhip_multi_refiner_create(C.byref(h), 0, 2, devs) == -1
    assert vaqlib.vaqhip_multi_refiner_create(C.byref(h), 8, 0, devs) == -1
    assert vaqlib.vaqhip_multi_refiner_create(C.byref(h), 8, 17, devs) == -1
    assert vaqlib.vaqhip_multi_refiner_create(C.byref(h), 1 << 20, 2, devs) == -2  # beyond the workgroup's LDS
    assert vaqlib.vaqhip_multi_last_error()
    assert vaqlib.vaqhip_multi_refiner_refine(None, None, 1, None, 1, 1, None, None) == -1
    assert vaqlib.vaqhip_multi_refiner_get_info(None, None) == -1
    vaqlib.vaqhip_multi_refiner_destroy(None)
    if vaqlib.vaqhip_device_count() <= 0:
        assert vaqlib.vaqhip_multi_refiner_create(C.byref(h), 8, 2, devs) == -3  # VAQHIP_ENODEVICE
        assert not h.value
        import vaq_amd
        with pytest.raises(vaq_amd.VaqHipError) as e:
            vaq_amd.VaqMultiRefiner([0, 0], 8)
        assert e.value.code == -3
