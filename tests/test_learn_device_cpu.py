"""CPU tests of learnQuantization's device forms: the symbols, what is refused before a device is touched, the Python
argument checks, and the host arithmetic of vaq_amd/csrc/learn_plan.h through its stand-alone program
(tests/cpp/learn_plan_test.cpp, once more under AddressSanitizer + UBSan: host code only, its own main)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fast_ref as fr
import learn_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vaqhip_learn_quantization_u8", "vaqhip_learn_quantization_device", "vaqhip_learn_quantization_u8_device",
       "vaqhip_learn_quantization_from_refiner", "vaqhip_multi_learn_quantization_u8",
       "vaqhip_multi_learn_quantization_from_refiner", "vaqhip_learn_set_workspace", "vaqhip_last_learn_timing"]


def _build(tmp_path, name, extra=()):
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "vaq_amd", "csrc")] + list(extra) +
                          [os.path.join(ROOT, "tests", "cpp", "learn_plan_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("learn_plan"), "learn_plan_test")


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")


def test_symbols_and_version(vaqlib):
    from vaq_amd import _lib
    assert vaqlib.vaqhip_version() >= 119
    for name in NEW:
        assert hasattr(vaqlib, name) and name in _lib.SYMBOLS
    t = _lib.LearnTiming()
    assert C.sizeof(t) == 3 * 4 + 6 * 4 + 4 + 7 * 8  # three ints, six floats, padding to 8, seven doubles


def test_refused_before_a_device_is_touched(vaqlib):
    """a null index or refiner is EINVAL in every form, as in the float forms"""
    one = np.zeros((4, 8), np.float32)
    b = np.zeros((4, 8), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    r = C.c_float(0.5)
    assert vaqlib.vaqhip_learn_quantization(None, p(one), 4, 0, r, None, None) == -1
    assert vaqlib.vaqhip_learn_quantization_u8(None, p(b), 4, 0, r, None, None) == -1
    assert vaqlib.vaqhip_learn_quantization_device(None, p(one), 4, 0, r, None, None) == -1
    assert vaqlib.vaqhip_learn_quantization_u8_device(None, p(b), 4, 0, r, None, None) == -1
    assert vaqlib.vaqhip_learn_quantization_from_refiner(None, None, r, None, None) == -1
    assert b"index is null" in vaqlib.vaqhip_last_error()
    assert vaqlib.vaqhip_multi_learn_quantization(None, p(one), 4, 0, r, None, None) == -1
    assert vaqlib.vaqhip_multi_learn_quantization_u8(None, p(b), 4, 0, r, None, None) == -1
    assert vaqlib.vaqhip_multi_learn_quantization_from_refiner(None, None, r, None, None) == -1
    assert b"multi index is null" in vaqlib.vaqhip_multi_last_error()
    assert vaqlib.vaqhip_last_learn_timing(None, None) == -1
    assert vaqlib.vaqhip_learn_set_workspace(-1) == -1
    assert vaqlib.vaqhip_learn_set_workspace(1 << 20) == 0
    assert vaqlib.vaqhip_learn_set_workspace(0) == 0


def test_python_u8_argument_checks():
    """a _u8 method takes a contiguous uint8 n x D array and nothing else: EINVAL before the library is reached"""
    import vaq_amd
    v = vaq_amd.VaqHipFast()
    v.mBitsAlloc = [4] * 4
    v.mCentroidsPerSubs = [np.zeros((16, 2), np.float32)] * 4
    good = np.zeros((20, 8), np.uint8)
    for bad in (good.astype(np.float32), good[:, ::2], good[::2].T, np.zeros((20, 7), np.uint8), np.zeros(8, np.uint8)):
        with pytest.raises(vaq_amd.VaqHipError) as e:
            v.learnQuantization_u8(bad, 0.5)
        assert e.value.code == -1
    for name in ("learnQuantization_device", "learnQuantization_u8_device", "learnQuantizationFromRefiner",
                 "last_learn_timing"):
        assert callable(getattr(vaq_amd.VaqHipFast, name))
    for name in ("learn_quantization_u8", "learn_quantization_from_refiner"):
        assert callable(getattr(vaq_amd.VaqHipMulti, name))


def test_plan_program(plan_exe):
    assert "learn_plan_test: ok" in _run(plan_exe, "self")


def test_plan_program_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "learn_plan_test_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    r = subprocess.run([exe, "self"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "learn_plan_test: ok" in r.stdout


@pytest.mark.parametrize("mc", [1, 3, 5, 8])
def test_column_groups_cover_every_subspace_once(plan_exe, mc):
    """budgets that give Mc = 1, an Mc that does not divide M, and Mc = M (group_bytes: Mc + 4 columns of values)"""
    sample, M, ksub = 257, 8, 16
    out = _run(plan_exe, "plan", sample * ksub * 4 * (mc + 4), sample, M, ksub)
    got_mc, groups = map(int, out[0].split())
    assert got_mc == mc and groups == -(-M // mc)
    seen = []
    for line in out[1:1 + groups]:
        s0, m = map(int, line.split())
        assert 1 <= m <= mc
        seen += list(range(s0, s0 + m))
    assert seen == list(range(M))


@pytest.mark.parametrize("rows", [16, 17, 640])
def test_percentile_over_an_accessor(plan_exe, tmp_path, rows):
    z = np.load(os.path.join(ROOT, "tests", "golden", "fast", "quantize.npz"))
    pcts = [np.float32(x) for x in z["pct_alphas"]] + [np.float32(1) - a for a in fr.ALPHAS]
    for j in (0, 5):
        col = np.sort(z["luts"][:rows, j]).astype(np.float32)
        f = tmp_path / f"col{j}.f32"
        col.tofile(f)
        out = _run(plan_exe, "percentile", f, rows, *[f"{float(x):.9g}" for x in pcts])
        got = np.array([int(x, 16) for x in out[:len(pcts)]], np.uint32).view(np.float32)
        want = np.array([fr.percentile(col, x) for x in pcts], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        if rows == 640:  # the reference's own values
            assert np.array_equal(got[:10], z["percentiles"][:, j])


class _Ramp:
    """v[i] = float32(i), never materialised"""
    def __init__(self, rows):
        self.shape = (rows,)

    def __getitem__(self, i):
        return np.float32(i)


@pytest.mark.parametrize("pct", [0.001, 0.005, 0.1, 0.9, 0.999])
def test_percentile_above_2_to_24_rows(plan_exe, pct):
    """nthF = percent * float(rows - 1) rounds in float there: the elements read are the checker's"""
    rows = (1 << 24) + 4_000_003
    out = _run(plan_exe, "percentile_ramp", rows, f"{float(np.float32(pct)):.9g}")[0].split()
    got = np.array([int(out[0], 16)], np.uint32).view(np.float32)[0]
    want = fr.percentile(_Ramp(rows), np.float32(pct))
    assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32)
    assert 0 <= int(out[2]) < rows and 0 <= int(out[3]) < rows


@pytest.mark.parametrize("rows", [1, 16, 1000, 4099])
def test_sequential_double_sum(plan_exe, tmp_path, rows):
    rng = np.random.default_rng(rows)
    col = (rng.random(rows) * 3000).astype(np.float32)
    col[rng.random(rows) < 0.2] = 0
    f = tmp_path / "col.f32"
    col.tofile(f)
    fl, sc = np.float32(17.25), np.float32(0.0931)
    out = _run(plan_exe, "loss", f, rows, f"{float(fl):.9g}", f"{float(sc):.9g}")
    got = np.array([int(out[0], 16)], np.uint64).view(np.float64)[0]
    terms = lr.column_terms(col, fl, sc)
    want = np.add.accumulate(terms, dtype=np.float64)[-1]
    assert got == want
