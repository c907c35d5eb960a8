"""The binary-tree codebook fit without a GPU: the oracle's own rules (tests/codebooks_bin_ref.py), what every case of
tests/test_codebooks_bin_gpu.py is there to reach, asserted from the oracle's tree, the host arithmetic of
vaq_amd/csrc/fit_codebooks_bin_plan.h through its stand-alone program, and the adapter's surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import codebooks_bin_ref as br
import codebooks_ref as cr
import kmeans_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the split rule ----------------------------------------------------------------------------------------------------
def test_tie_and_nan_go_right():
    C = np.array([[-1.0, 0.0], [1.0, 0.0]], np.float32)
    x = np.array([[0.0, 3.0], [-0.5, 0.0], [0.5, 0.0], [np.nan, 0.0], [np.inf, 0.0]], np.float32)
    assert list(br.goes_left(x, C)) == [False, True, False, False, False]  # tie, left, right, NaN, inf - inf = NaN


def test_split_compares_squares_not_roots():
    """The 1 / 1 + 2^-23 pair: the squares differ, their roots round to one float.  The split takes the smaller square
    wherever it stands; compared by roots the two would tie and the row would go right both times."""
    one, above = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0), dtype=np.float32)
    assert one != above and np.sqrt(one) == np.sqrt(above)
    x = np.zeros((1, 2), np.float32)
    far, near = [1.0, 2.0 ** -11.5], [1.0, 0.0]  # squares 1 + 2^-23 and 1
    d2 = br.sq_dist_eigen(x, np.array([far, near], np.float32))
    assert d2[0, 0] == above and d2[0, 1] == one
    assert not br.goes_left(x, np.array([far, near], np.float32))[0]
    assert br.goes_left(x, np.array([near, far], np.float32))[0]      # (by roots: a tie, right)
    assert kr.assign_full(x, np.array([far, near], np.float32))[0] == 0  # the Lloyd rule sees the tie


def test_nan_centre_sends_all_rows_right_and_the_node_is_cut():
    rng = np.random.default_rng(1)
    X = rng.normal(size=(100, 3)).astype(np.float32)
    for C in (np.array([[np.nan] * 3, [0.0] * 3], np.float32), np.array([[0.0] * 3, [np.nan] * 3], np.float32)):
        assert not br.goes_left(X, C).any()
    # equal seed rows: the second centre is empty after the first assign, NaN for ever; every row goes right; cut
    Xd = X.copy()
    a, b = kr.permutation_head(len(Xd), 2)
    Xd[b] = Xd[a]
    cents, tree = br.fit_subspace_bin(Xd, 3, cr.MAX_ITER)
    assert tree[0]["nan2"] and tree[0]["sizeleft"] == 0 and tree[0]["kind"] == br.CUT and len(tree) == 1
    want, it = kr.fit(Xd, 8, cr.MAX_ITER)
    cr.assert_centres_equal(cents, want, "a cut at the root is the flat fit")


@pytest.mark.parametrize("name", ["odd", "tiny"])
def test_no_wide_subspace_is_the_flat_fit(name):
    n, D, M, bits, kind, salt = cr.CASES[name]
    X, eig = cr.make_inputs(name)
    got = br.fit_codebooks_bin(X, M, bits, eig)
    want = cr.fit_codebooks(X, M, bits, eig)
    assert got[3] == {}
    for s in range(M):
        cr.assert_centres_equal(got[0][s], want[0][s], f"{name}, subspace {s}")
    assert list(got[1]) == list(want[1])


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _nodes(name):
    return [nd for t in br.expected(name)[3].values() for nd in t]


@pytest.mark.parametrize("name", list(br.CASES))
def test_case_is_a_valid_input(name):
    """Every binary subspace has a tree whose outputs tile its block: every centre was written (no sentinel left), every
    node holds at least tempK rows, the children of a split node share its rows, the level order is (depth, index)."""
    n, D, M, bits, kind, salt = br.CASES[name]
    cents, iters, nans, trees = br.expected(name)
    assert sorted(trees) == [s for s in range(M) if br.binary(bits[s])] and trees
    for s, tree in trees.items():
        assert cents[s].shape == (1 << bits[s], D // M) and not (cents[s] == np.float32(-12345.0)).any()
        assert tree[0]["rows"] == br.rows_for(n, bits[s], sum(bits), M) and tree[0]["depth"] == 1
        by = {(nd["depth"], nd["index"]): nd for nd in tree}
        covered = 0
        for nd in tree:
            tempK = 1 << (bits[s] - nd["depth"] + 1)
            assert nd["rows"] >= tempK
            if nd["kind"] == br.SPLIT:
                assert nd["sizeleft"] + nd["sizeright"] == nd["rows"] and min(nd["sizeleft"], nd["sizeright"]) >= tempK // 2
                assert by[(nd["depth"] + 1, 2 * nd["index"])]["rows"] == nd["sizeleft"]
                assert by[(nd["depth"] + 1, 2 * nd["index"] + 1)]["rows"] == nd["sizeright"]
            else:
                covered += tempK
                assert (nd["kind"] == br.LEAF) == (nd["depth"] == bits[s])
        assert covered == 1 << bits[s]
        assert iters[s] == max(max(nd["iters"], nd.get("cut_iters", 0)) for nd in tree)


def test_cases_cover_what_the_table_names():
    every = {name: _nodes(name) for name in br.CASES}
    # a path that reaches leaf depth; a cut below the root (`tiny`: at the deep levels)
    assert any(nd["kind"] == br.LEAF for nd in every["tiny"])
    assert any(nd["kind"] == br.CUT and nd["depth"] >= 5 for nd in every["tiny"])
    assert len(br.expected("l1")[3]) == 2 and br.CASES["l1"][1] // br.CASES["l1"][2] == 1
    assert br.CASES["l12"][0] % 2 == 1 and br.CASES["l12"][1] == 12          # odd rows_s, a packet and a tail of 4
    assert br.CASES["wide"][1] > 64                                          # more columns than lanes
    # a cut AT the root: the subspace is the flat fit of its rows
    n, D, M, bits, kind, salt = br.CASES["rootcut"]
    root = every["rootcut"][0]
    assert len(every["rootcut"]) == 1 and root["kind"] == br.CUT and min(root["sizeleft"], root["sizeright"]) < 256
    X, _ = br.inputs("rootcut")
    want, it = kr.fit(X[kr.permutation_head(n, n)], 512, cr.MAX_ITER)
    cr.assert_centres_equal(br.expected("rootcut")[0][0], want, "rootcut")
    # a 2-centre fit that samples, with a child above 65536 rows that samples again
    res = [nd for nd in every["resampled"] if nd["sampled"]]
    assert [nd["depth"] for nd in res] == [1, 2] and all(nd["rows"] > 65536 for nd in res) and res[0]["kind"] == br.SPLIT
    # a cut fit that samples: m > max(256 tempK, 65536)
    cs = [nd for nd in every["cutsampled"] if nd.get("cut_sampled")]
    assert len(cs) == 1 and cs[0]["rows"] > max(256 << (9 - cs[0]["depth"] + 1), 65536)
    # a NaN 2-centre centre that forces a cut; a NaN centre that survives to the output; B / M decides rows_s
    assert any(nd["nan2"] and nd["kind"] == br.CUT and nd["sizeleft"] == 0 for nd in every["paired"])
    assert all(np.isnan(c).any() for c in br.expected("paired")[0])
    n, D, M, bits, kind, salt = br.CASES["paired"]
    assert sum(bits) // M == 10 and (256 << 10) > 256 << bits[0] and br.rows_for(n, bits[0], sum(bits), M) == n
    # nodes of odd and of even size; a fit that runs to max_iter and one that stops by itself
    for name, nodes in every.items():
        if len(nodes) > 1:
            assert any(nd["rows"] % 2 for nd in nodes) and any(nd["rows"] % 2 == 0 for nd in nodes), name
    its = [nd["iters"] for nodes in every.values() for nd in nodes]
    assert max(its) == cr.MAX_ITER and min(its) < cr.MAX_ITER
    X8, eig = br.byte_inputs()
    assert X8.dtype == np.uint8 and X8.max() == 255


# ---- fit_codebooks_bin_plan.h ------------------------------------------------------------------------------------------
def _build(tmp_path, name, extra=()):
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "vaq_amd", "csrc")] + list(extra) +
                          [os.path.join(ROOT, "tests", "cpp", "fit_codebooks_bin_plan_test.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fit_codebooks_bin_plan"), "fit_codebooks_bin_plan_test")


def test_plan_program(plan_exe):
    assert "fit_codebooks_bin_plan_test: ok" in _run(plan_exe, "self")


def test_plan_program_under_sanitizers(tmp_path):
    """a plain executable with the sanitizers linked in, run directly"""
    exe = _build(tmp_path, "fit_codebooks_bin_plan_test_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                                               "-fno-sanitize-recover=undefined"])
    assert "fit_codebooks_bin_plan_test: ok" in _run(exe, "self")


@pytest.mark.parametrize("name", list(br.CASES))
def test_plan_of_every_case(plan_exe, name):
    """the binary subspaces, their rows and blocks as the oracle has them"""
    n, D, M, bits, kind, salt = br.CASES[name]
    out = [list(map(int, line.split())) for line in _run(plan_exe, "rows", n, M, ",".join(map(str, bits))) if line]
    assert [o[0] for o in out] == [s for s in range(M) if br.binary(bits[s])]
    for s, b, k, rows, cent_off in out:
        assert (b, k, rows) == (bits[s], 1 << bits[s], br.rows_for(n, bits[s], sum(bits), M))
        assert cent_off == sum(1 << x for x in bits[:s])


# ---- the adapter -------------------------------------------------------------------------------------------------------
def test_adapter_names_and_early_refusals():
    import vaq_amd
    from vaq_amd import _lib
    for name in ("fit_codebooks_bin", "fit_codebooks_bin_u8", "last_fit_codebooks_bin_timing"):
        assert name in vaq_amd.__all__ and callable(getattr(vaq_amd, name))
    assert callable(vaq_amd.VaqRefiner.fit_codebooks_bin) and not hasattr(vaq_amd.VaqMultiRefiner, "fit_codebooks_bin")
    for sym in ("vaqhip_fit_codebooks_bin", "vaqhip_fit_codebooks_bin_device", "vaqhip_fit_codebooks_bin_u8",
                "vaqhip_fit_codebooks_bin_u8_device", "vaqhip_refiner_fit_codebooks_bin", "vaqhip_last_fit_codebooks_bin_timing",
                "vaqhip_fit_codebooks_bin_set_sums"):
        assert sym in _lib.SYMBOLS
    with pytest.raises(vaq_amd.VaqHipError) as e:  # (refused by the adapter: no library call)
        vaq_amd.fit_codebooks_bin(np.zeros((600, 4), np.float32), 2, [9])
    assert e.value.code == -1
    with pytest.raises(vaq_amd.VaqHipError) as e:
        vaq_amd.fit_codebooks_bin_u8(np.zeros((600, 4), np.float32), 2, [9, 3])
    assert e.value.code == -1
