"""The CPU side of the encode across the shards of a multi-device index (vaqhip_multi_encode_set_codes, _add_codes,
_from_refiner, vaqhip_multi_last_encode_timing): the symbols, and the refusals that are made before the index, the
refiner or any device is touched.  What needs an index (labels past int32, ESTATE, mismatched devices) is in
tests/test_encode_multi_gpu.py."""
import ctypes as C

NEW_SYMBOLS = ("vaqhip_multi_encode_set_codes", "vaqhip_multi_encode_add_codes", "vaqhip_multi_encode_from_refiner",
               "vaqhip_multi_last_encode_timing")


def test_symbols_and_version(vaqlib):
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 115
    for s in NEW_SYMBOLS:
        assert hasattr(vaqlib, s) and s in _lib.SYMBOLS, s
    assert [f for f, _ in _lib.MultiEncodeTiming._fields_] == ["total_ms", "encode_ms", "set_codes_ms", "rows", "n_devices"]
    from vaq_amd.index import VaqHipMulti
    for m in ("encode", "encode_add", "encode_from_refiner", "last_encode_timing"):
        assert callable(getattr(VaqHipMulti, m)), m


def test_refusals_without_a_device(vaqlib):
    """EINVAL (-1) before anything is dereferenced: p is never read on these paths"""
    p = C.c_void_p(64)
    s, a, r = (vaqlib.vaqhip_multi_encode_set_codes, vaqlib.vaqhip_multi_encode_add_codes,
               vaqlib.vaqhip_multi_encode_from_refiner)
    assert s(None, p, 10, 1, 0, None) == -1 and b"null" in vaqlib.vaqhip_multi_last_error()
    assert s(p, None, 10, 1, 0, None) == -1
    assert s(p, p, -1, 1, 0, None) == -1
    assert s(p, p, 10, 1, -1, None) == -1
    assert s(p, p, 10, 0, -5, p) == -1
    assert a(None, p, 10, 1, None) == -1
    assert a(p, None, 10, 1, None) == -1
    assert a(p, p, -1, 1, None) == -1
    assert r(None, p, None) == -1
    assert r(p, None, None) == -1 and b"refiner" in vaqlib.vaqhip_multi_last_error()
    assert r(None, None, p) == -1
    from vaq_amd import _lib
    assert vaqlib.vaqhip_multi_last_encode_timing(None, C.byref(_lib.MultiEncodeTiming())) == -1
    assert vaqlib.vaqhip_multi_last_encode_timing(p, None) == -1


def test_encode_chunk_rows_refusals(vaqlib):
    """a negative chunk is refused before the index is locked; so is a null index or key"""
    p = C.c_void_p(64)
    so = vaqlib.vaqhip_multi_set_option
    assert so(p, b"encode_chunk_rows", -1) == -1 and b"encode_chunk_rows" in vaqlib.vaqhip_multi_last_error()
    assert so(p, b"encode_chunk_rows", -(1 << 40)) == -1
    assert so(None, b"encode_chunk_rows", 100) == -1
    assert so(p, None, 100) == -1
