"""The hierarchical codebook fit without a GPU: the oracle's own rules (tests/codebooks_hier_ref.py), the conditions that
make every case of tests/test_codebooks_hier_gpu.py a valid input, the host arithmetic of
vaq_amd/csrc/fit_codebooks_hier_plan.h through its stand-alone program, and the adapter's surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import codebooks_hier_ref as hr
import codebooks_ref as cr
import kmeans_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_membership_compares_squares_not_roots():
    """Two distinct squared distances whose square roots round to one float: the membership rule (no sqrt) takes the
    smaller square, the Lloyd rule (sqrt, strict <, centres ascending) the first centre."""
    one, above = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0), dtype=np.float32)  # 1 + 2^-23
    assert one != above and np.sqrt(one) == np.sqrt(above)
    x = np.zeros((1, 2), np.float32)
    C = np.array([[1.0, 2.0 ** -11.5], [1.0, 0.0]], np.float32)  # squares 1 + 2^-23 and 1
    d2 = hr.sq_dist_eigen(x, C)
    assert d2[0, 0] == above and d2[0, 1] == one
    g, lost = hr.membership(x, C)
    assert g[0] == 1 and not lost.any()      # the smaller square
    assert kr.assign_full(x, C)[0] == 0      # the roots tie: the first centre
    # a row at a NaN or huge distance from every centre has no centre
    g, lost = hr.membership(np.array([[np.inf, 0.0]], np.float32), C)
    assert lost.all()


def test_rows_of_a_hierarchical_subspace():
    assert hr.rows_for(1000000, 12, 64, 8) == 1000000
    assert hr.rows_for(10000000, 9, 80, 8) == 256 << 10    # 256 << (B / M) above 256 * k_s
    assert hr.rows_for(10000000, 9, 87, 8) == 256 << 10    # integer division
    assert hr.rows_for(10000000, 12, 64, 8) == 256 << 12
    n, D, M, bits, kind, salt = hr.CASES["budget"]
    assert sum(bits) // M == 10 and (256 << 10) > 256 << bits[0] and hr.rows_for(n, bits[0], sum(bits), M) == n


@pytest.mark.parametrize("name", ["odd", "tiny"])
def test_no_wide_subspace_is_the_flat_fit(name):
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = cr.make_inputs(name)
    got = hr.fit_codebooks_hier(X, M, bits, eig)
    want = cr.fit_codebooks(X, M, bits, eig)
    assert got[3] == {}
    for s in range(M):
        cr.assert_centres_equal(got[0][s], want[0][s], f"{name}, subspace {s}")
    assert list(got[1]) == list(want[1])


@pytest.mark.parametrize("name", list(hr.CASES))
def test_case_is_a_valid_input(name):
    """What keeps the reference's rule inside its own bounds: no NaN stage-1 centre, every row has a centre, every group
    holds at least K2 rows and at most max(256 K2, 65536), groups of odd and of even size occur."""
    n, D, M, bits, kind, salt = hr.CASES[name]
    cents, iters, nans, info = hr.expected(name)
    assert sorted(info) == [s for s in range(M) if hr.hierarchical(bits[s])] and info
    for s, d in info.items():
        assert not np.isnan(d["C1"]).any(), (name, s)
        assert d["lost"] == 0
        assert d["sizes"].sum() == hr.rows_for(n, bits[s], sum(bits), M)
        assert d["sizes"].min() >= d["K2"] and d["sizes"].max() <= hr.group_limit(d["K2"]), (name, s, d["sizes"].min())
        assert (d["sizes"] % 2 == 1).any() and (d["sizes"] % 2 == 0).any()
        assert cents[s].shape == (1 << bits[s], D // M) and len(d["it2"]) == hr.K1
        assert iters[s] == max([d["it1"]] + d["it2"])


def test_cases_cover_what_the_table_names():
    it2 = {name: [it for d in hr.expected(name)[3].values() for it in d["it2"]] for name in hr.CASES}
    assert any(max(v) == cr.MAX_ITER for v in it2.values())          # a stage-2 fit that runs to max_iter ...
    assert any(min(v) < cr.MAX_ITER for v in it2.values())           # ... and ones that stop by themselves
    assert np.isnan(hr.expected("budget")[0][1]).any()               # a NaN centre of a stage-2 fit survives to the output
    n, D, M, bits, kind, salt = hr.CASES["resampled"]
    assert cr.sample_count(n, hr.K1) == 65536 < n                    # stage 1 samples for itself
    assert hr.CASES["l12"][0] % 2 == 1 and hr.CASES["l12"][1] == 12  # odd rows_s, a packet and a tail of 4
    sizes = hr.expected("l12")[3][0]["sizes"]
    assert sizes.min() >= 28                                         # planted: the groups are the blobs
    X8, eig = hr.byte_inputs()
    assert X8.dtype == np.uint8 and X8.max() == 255 and all(c is not None for c in hr.expected_bytes()[0])


# ---- fit_codebooks_hier_plan.h -------------------------------------------------------------------------------------
def _build(tmp_path, name, extra=()):
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "vaq_amd", "csrc")] + list(extra) +
                          [os.path.join(ROOT, "tests", "cpp", "fit_codebooks_hier_plan_test.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fit_codebooks_hier_plan"), "fit_codebooks_hier_plan_test")


def test_plan_program(plan_exe):
    assert "fit_codebooks_hier_plan_test: ok" in _run(plan_exe, "self")


def test_plan_program_under_sanitizers(tmp_path):
    """a plain executable with the sanitizers linked in, run directly"""
    exe = _build(tmp_path, "fit_codebooks_hier_plan_test_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                                                "-fno-sanitize-recover=undefined"])
    assert "fit_codebooks_hier_plan_test: ok" in _run(exe, "self")


@pytest.mark.parametrize("name", list(hr.CASES))
def test_plan_of_every_case(plan_exe, name):
    """rows, stage-1 rows and offsets of the hierarchical subspaces as the oracle has them"""
    n, D, M, bits, kind, salt = hr.CASES[name]
    out = [list(map(int, line.split())) for line in _run(plan_exe, "rows", n, M, ",".join(map(str, bits))) if line]
    hier = [s for s in range(M) if hr.hierarchical(bits[s])]
    assert [o[0] for o in out] == hier
    pair = 0
    for i, (s, k, K2, rows, stage1_rows, resampled, c1_off, pair_off) in enumerate(out):
        want = hr.rows_for(n, bits[s], sum(bits), M)
        assert (k, K2, rows) == (1 << bits[s], 1 << (bits[s] - 7), want)
        assert stage1_rows == cr.sample_count(want, hr.K1) and resampled == int(want > 65536)
        assert c1_off == sum(1 << b for b in bits) + 128 * i and pair_off == pair
        pair += rows


# ---- the adapter -----------------------------------------------------------------------------------------------------
def test_adapter_names_and_early_refusals():
    import vaq_amd
    from vaq_amd import _lib
    for name in ("fit_codebooks_hier", "fit_codebooks_hier_u8", "last_fit_codebooks_hier_timing"):
        assert name in vaq_amd.__all__ and callable(getattr(vaq_amd, name))
    assert callable(vaq_amd.VaqRefiner.fit_codebooks_hier) and not hasattr(vaq_amd.VaqMultiRefiner, "fit_codebooks_hier")
    for sym in ("vaqhip_fit_codebooks_hier", "vaqhip_fit_codebooks_hier_device", "vaqhip_fit_codebooks_hier_u8",
                "vaqhip_fit_codebooks_hier_u8_device", "vaqhip_refiner_fit_codebooks_hier", "vaqhip_last_fit_codebooks_hier_timing"):
        assert sym in _lib.SYMBOLS
    with pytest.raises(vaq_amd.VaqHipError) as e:  # (refused by the adapter: no library call)
        vaq_amd.fit_codebooks_hier(np.zeros((600, 4), np.float32), 2, [9])
    assert e.value.code == -1
    with pytest.raises(vaq_amd.VaqHipError) as e:
        vaq_amd.fit_codebooks_hier_u8(np.zeros((600, 4), np.float32), 2, [9, 3])
    assert e.value.code == -1
