"""The CPU side of building an index from byte rows (the *_u8 forms of encode, encode_lut and the quantile fits): the
exported symbols, the refusals that need no device -- each with its float twin's code --, the Python methods, and that
a _u8 method converts nothing."""
import ctypes as C
import os

import numpy as np
import pytest

# (byte form, its float twin)
TWINS = (("vaqhip_encode_u8", "vaqhip_encode"), ("vaqhip_encode_u8_device", "vaqhip_encode_device"),
         ("vaqhip_encode_lut_u8", "vaqhip_encode_lut"), ("vaqhip_encode_lut_u8_device", "vaqhip_encode_lut_device"),
         ("vaqhip_lut_fit_quantiles_u8", "vaqhip_lut_fit_quantiles"),
         ("vaqhip_lut_fit_quantiles_u8_device", "vaqhip_lut_fit_quantiles_device"),
         ("vaqhip_multi_encode_set_codes_u8", "vaqhip_multi_encode_set_codes"),
         ("vaqhip_multi_encode_add_codes_u8", "vaqhip_multi_encode_add_codes"),
         ("vaqhip_multi_encode_lut_set_codes_u8", "vaqhip_multi_encode_lut_set_codes"),
         ("vaqhip_multi_encode_lut_add_codes_u8", "vaqhip_multi_encode_lut_add_codes"),
         ("vaqhip_multi_lut_fit_quantiles_u8", "vaqhip_multi_lut_fit_quantiles"))


def test_symbols_and_version(vaqlib):
    import vaq_amd
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 118
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vaqhip.h")).read()
    for s, twin in TWINS:
        assert hasattr(vaqlib, s) and s in _lib.SYMBOLS, s
        assert f"int {s}(" in header, s
        assert getattr(vaqlib, s).argtypes == getattr(vaqlib, twin).argtypes, s
    for m in ("encode_u8", "encode_u8_device", "fitQuantiles_u8", "encodeLUT_u8", "encodeLUT_u8_device"):
        assert callable(getattr(vaq_amd.VaqHip, m)), m
    for m in ("encode_u8", "encode_add_u8", "encode_lut_u8", "encode_lut_add_u8"):
        assert callable(getattr(vaq_amd.VaqHipMulti, m)), m
    assert callable(vaq_amd.lut_fit_quantiles_multi_u8) and "lut_fit_quantiles_multi_u8" in vaq_amd.__all__
    assert "no byte form yet" not in header and "does not yet" not in header


def test_refusals_touch_no_device(vaqlib):
    """Every byte entry refuses what its float twin refuses, with the twin's code, before a handle is read or a device
    touched: p is never dereferenced on these paths."""
    L = vaqlib
    p = C.c_void_p(64)
    for u8, f32 in ((L.vaqhip_encode_u8, L.vaqhip_encode), (L.vaqhip_encode_lut_u8, L.vaqhip_encode_lut)):
        for f in (u8, f32):
            assert f(None, p, 4, 0, p) == -1 and b"null" in L.vaqhip_last_error()
            assert f(None, p, -1, 0, p) == -1
    for u8, f32 in ((L.vaqhip_encode_u8_device, L.vaqhip_encode_device),
                    (L.vaqhip_encode_lut_u8_device, L.vaqhip_encode_lut_device)):
        for f in (u8, f32):
            assert f(None, p, 4, 0, p, None) == -1 and b"null" in L.vaqhip_last_error()
    ok = (C.c_int * 3)(8, 3, 1)
    bad_bits = (C.c_int * 3)(8, 9, 1)
    zero_bits = (C.c_int * 3)(8, 0, 1)
    for u8, f32 in ((L.vaqhip_lut_fit_quantiles_u8, L.vaqhip_lut_fit_quantiles),):
        for f in (u8, f32):
            assert f(0, None, 4, 3, ok, None, p, p) == -1 and b"null" in L.vaqhip_last_error()
            assert f(0, p, 4, 3, None, None, p, p) == -1
            assert f(0, p, 4, 3, ok, None, None, p) == -1
            assert f(0, p, 4, 3, ok, None, p, None) == -1
            assert f(0, p, -1, 3, ok, None, p, p) == -1
            assert f(0, p, 0, 3, ok, None, p, p) == -1
            assert f(0, p, 1 << 31, 3, ok, None, p, p) == -1
            assert f(0, p, 4, 0, ok, None, p, p) == -1
            assert f(0, p, 4, 4097, ok, None, p, p) == -2  # EUNSUPPORTED, as the float fit
            assert f(0, p, 4, 3, bad_bits, None, p, p) == -1 and b"bits[1]=9" in L.vaqhip_last_error()
            assert f(0, p, 4, 3, zero_bits, None, p, p) == -1
    for u8, f32 in ((L.vaqhip_lut_fit_quantiles_u8_device, L.vaqhip_lut_fit_quantiles_device),):
        for f in (u8, f32):
            assert f(0, None, 4, 3, ok, None, p, p, None) == -1
            assert f(0, p, -1, 3, ok, None, p, p, None) == -1
            assert f(0, p, 4, 4097, ok, None, p, p, None) == -2
            assert f(0, p, 4, 3, bad_bits, None, p, p, None) == -1
    err = L.vaqhip_multi_last_error
    for u8, f32 in ((L.vaqhip_multi_encode_set_codes_u8, L.vaqhip_multi_encode_set_codes),
                    (L.vaqhip_multi_encode_lut_set_codes_u8, L.vaqhip_multi_encode_lut_set_codes)):
        for f in (u8, f32):
            assert f(None, p, 4, 0, 0, None) == -1 and b"null" in err()
    for u8, f32 in ((L.vaqhip_multi_encode_add_codes_u8, L.vaqhip_multi_encode_add_codes),
                    (L.vaqhip_multi_encode_lut_add_codes_u8, L.vaqhip_multi_encode_lut_add_codes)):
        for f in (u8, f32):
            assert f(None, p, 4, 0, None) == -1 and b"null" in err()
    devs = (C.c_int * 2)(0, 0)
    for f in (L.vaqhip_multi_lut_fit_quantiles_u8, L.vaqhip_multi_lut_fit_quantiles):
        assert f(2, devs, None, 4, 3, ok, None, p, p) == -1 and b"null" in err()
        assert f(2, None, p, 4, 3, ok, None, p, p) == -1
        assert f(2, devs, p, 4, 3, None, None, p, p) == -1
        assert f(2, devs, p, 4, 3, ok, None, None, p) == -1
        assert f(2, devs, p, -1, 3, ok, None, p, p) == -1
        assert f(2, devs, p, 1 << 31, 3, ok, None, p, p) == -1
        assert f(2, devs, p, 4, 4097, ok, None, p, p) == -2
        assert f(2, devs, p, 4, 3, bad_bits, None, p, p) == -1 and b"bits[1]=9" in err()
        assert f(0, devs, p, 4, 3, ok, None, p, p) == -1 and b"n_devices" in err()
        assert f(17, devs, p, 4, 3, ok, None, p, p) == -1


def test_u8_methods_convert_nothing(vaqlib):
    """A float array (or a byte array of the wrong shape, or one that is not contiguous) into a _u8 method is EINVAL,
    decided on the host before any handle exists."""
    import vaq_amd
    Xf = np.zeros((6, 4), np.float32)
    Xi = np.zeros((6, 4), np.int8)
    wide = np.zeros((6, 8), np.uint8)
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = [3, 2, 1, 4]
    v.mCentroidsPerSubs = [np.zeros((1 << b, 1), np.float32) for b in v.mBitsAlloc]
    v.mQuantiles = np.zeros((4, 257), np.float32)
    calls = [v.encode_u8, v.fitQuantiles_u8, v.encodeLUT_u8, lambda X: v.fitQuantiles_u8(X, devices=[0, 0]),
             lambda X: vaq_amd.lut_fit_quantiles_multi_u8([0, 0], X, [3, 2, 1, 4])]
    for call in calls:
        for X in (Xf, Xi, wide[:, ::2], Xf.tolist()):
            with pytest.raises(vaq_amd.VaqHipError) as e:
                call(X)
            assert e.value.code == -1 and "uint8" in str(e.value), (call, type(X))
    for call in calls[:3]:
        with pytest.raises(vaq_amd.VaqHipError) as e:
            call(wide)
        assert e.value.code == -1
    m = vaq_amd.VaqHipMulti.__new__(vaq_amd.VaqHipMulti)  # (no handle: the refusal comes before it is read)
    m._h, m.D, m.M = C.c_void_p(), 4, 4
    for call in (m.encode_u8, m.encode_add_u8, m.encode_lut_u8, m.encode_lut_add_u8):
        for X in (Xf, Xi, wide):
            with pytest.raises(vaq_amd.VaqHipError) as e:
                call(X)
            assert e.value.code == -1
