"""FAST search method without a GPU: the NumPy checker (tests/fast_ref.py) against
fixtures recorded from the reference's own functions (tests/golden/fast/README.md),
and the host-side argument checks of vaq_amd.VaqHipFast."""
import os

import numpy as np
import pytest

import fast_ref as fr
import vaq_amd
from vaq_amd import NNMethod, VaqHipError

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast")


def _load(name):
    return np.load(os.path.join(GOLD, name))


@pytest.mark.parametrize("i", range(7))
def test_knn_from_dists_matches_reference(i):
    g = _load("knn_from_dists.npz")
    d, k = g[f"d{i}"], int(g[f"k{i}"])
    lab, dis = fr.knn_from_dists(d, k)
    assert np.array_equal(lab, g[f"labels{i}"].astype(np.int64))
    assert np.array_equal(dis, g[f"dists{i}"].astype(np.float32))


def test_std_sort_restatement_is_not_stable():
    """the head order is std::sort's, not a stable sort's: with > 16 equal keys
    libstdc++ reorders them, and so must the checker"""
    g = _load("knn_from_dists.npz")
    d = g["d5"][:1000]  # all equal
    perm = fr.std_sort_perm(d)
    assert sorted(perm.tolist()) == list(range(1000))
    assert not np.array_equal(perm, np.arange(1000))
    assert np.array_equal(perm, g["labels5"][:1000])


def test_random_permutation_matches_reference():
    g = _load("random_permutation.npz")
    assert np.array_equal(fr.random_permutation(37), g["perm37"])
    assert np.array_equal(fr.random_permutation(1000), g["perm1000"])
    assert np.array_equal(fr.random_permutation(100000)[:4000], g["perm100000_head"])


def test_percentile_matches_reference():
    g = _load("quantize.npz")
    for a, row in zip(g["pct_alphas"], g["percentiles"]):
        assert np.array_equal(fr.percentile_cols(g["luts"], a), row), a


def test_small_quantize_matches_reference():
    g = _load("quantize.npz")
    luts = g["luts"]
    a = np.float32(0.01)
    floors = fr.percentile_cols(luts, a)
    off = np.maximum(luts - floors[None, :], np.float32(0))
    sc = (np.float32(255) / fr.percentile_cols(off, np.float32(1) - a)).astype(np.float32)
    # small_quantize works on [M][rows]: the offset is already applied, so pass zeros
    q = fr.small_quantize(off.T, np.zeros(luts.shape[1], np.float32), sc).T
    assert np.array_equal(q, g["quantized_alpha01"])
    # and with the offsets applied inside (VAQ.cpp:1782-1789)
    assert np.array_equal(fr.small_quantize(luts.T, floors, sc).T, g["quantized_alpha01"])


def test_learn_alpha_loop_matches_reference():
    g = _load("quantize.npz")
    off, sc, _ = fr.learn_from_luts(g["luts"])
    assert np.array_equal(off, g["offsets"])
    assert np.array_equal(sc, g["scale"])


def test_row_sum_matches_reference():
    g = _load("row_sum.npz")
    n = g["dists"].shape[0]
    codes = g["codes_cmajor"][:n]
    small = g["small"].copy()
    for s, nc in enumerate(g["ncent"]):  # the reference copies mCentroidsNum[s] entries only
        small[s, nc:] = 0
    assert np.array_equal(fr.row_dists(small, codes), g["dists"].astype(np.int64))


# ------------------------------------------------------------------ the mirror's checks --
def test_fast_parse_method_string():
    v = vaq_amd.VaqHipFast()
    v.parseMethodString("VAQ256m64min4max4var1,FAST")
    assert v.mMethods == NNMethod.Fast and v.mMaxBitsPerSubs == 4
    v.parseMethodString("VAQ256m64min1max4var1,HEAP_FAST")
    assert v.mMethods == NNMethod.Heap | NNMethod.Fast
    with pytest.raises(VaqHipError) as e:
        v.parseMethodString("VAQ256m32min8max8var1,FAST")
    assert e.value.code == -2
    for bad in ("VAQ256m64min4max4var1,SORT", "VAQ256m64min4max4var1,FAST2", "VAQ256m64min4max4var1,FAST3"):
        with pytest.raises(VaqHipError):
            vaq_amd.VaqHipFast().parseMethodString(bad)


def test_plain_vaqhip_still_refuses_fast():
    with pytest.raises(VaqHipError):
        vaq_amd.VaqHip().parseMethodString("VAQ256m64min4max4var1,FAST")


def test_fast_quantization_argument_checks():
    v = vaq_amd.VaqHipFast()
    v.mBitsAlloc = [4] * 8
    with pytest.raises(VaqHipError):
        v.setLUTQuantization(np.zeros(7, np.float32), np.ones(8, np.float32))
    with pytest.raises(VaqHipError):
        v.setLUTQuantization(np.zeros(8, np.float32), np.zeros(8, np.float32))
    with pytest.raises(VaqHipError):
        v.setLUTQuantization(np.full(8, np.nan, np.float32), np.ones(8, np.float32))
    with pytest.raises(VaqHipError):
        v.setLUTQuantization(np.zeros(8, np.float32), np.full(8, np.inf, np.float32))
    v.setLUTQuantization(np.zeros(8), np.ones(8))
    assert v.mOffsets.dtype == np.float32 and v.mScale.shape == (8,)
    with pytest.raises(VaqHipError) as e:
        v.learnQuantization(np.zeros((9, 16), np.float32), 0.1)  # int(0.1 * 9) = 0 rows
    assert e.value.code == -1


# ------------------------------------------- the std::sort restatements against libstdc++ --
def _stdsort_sequences():
    import stdsort_cases as sc
    seqs = sc.shaped_sequences()
    adv = sc.adversarial_sequences()
    seqs += [(name, keys) for name, _, keys in adv]
    return seqs, adv


def test_stdsort_restatements_match_libstdcxx(tmp_path):
    """vaq::stdsort::sort (vaq_fast.h, built for the host) and fast_ref.std_sort_perm against the real
    std::sort over KNNFromDists' element and comparator, permutation for permutation: every n in
    1..1024, few-valued / organ-pipe / sawtooth / sorted keys, and adversarial sequences that reach the
    heap-sort fallback (asserted, with the sub-range lengths, on the checker's replay)."""
    import shutil
    import subprocess
    import stdsort_cases as sc
    seqs, adv = _stdsort_sequences()
    assert {len(k) for _, k in seqs} >= set(range(1, 1025))
    assert all(0 <= int(k.min()) and int(k.max()) <= 1024 for _, k in seqs)
    assert {n for _, n, _ in adv} >= {64, 100, 257, 1000, 1023, 1024}
    reached = []
    for name, n, keys in adv:
        assert n >= 64 and len(keys) == n
        lengths = sc.reaches_heap_sort(keys)
        assert len(lengths) >= 1 and all(ln > 16 for ln in lengths), (name, lengths)
        reached += lengths
    assert any(ln % 2 == 0 for ln in reached) and any(ln % 2 == 1 for ln in reached)  # adjust_heap's even tail
    assert any(len(np.unique(keys)) < n // 2 for _, n, keys in adv)                     # ... and equal keys in it

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / "stdsort_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(root, "vaq_amd", "csrc"), os.path.join(root, "tests", "cpp", "stdsort_test.cpp"),
                           "-o", exe])
    blob = [np.array([len(seqs)], np.int32)]
    for _, keys in seqs:
        blob += [np.array([len(keys)], np.int32), keys.astype(np.int32)]
    np.concatenate(blob).tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"stdsort_test: ok ({len(seqs)} sequences)" in r.stdout
    perms = np.fromfile(str(tmp_path / "out.bin"), np.int32)
    assert perms.size == sum(len(k) for _, k in seqs)
    at = 0
    for name, keys in seqs:
        want = perms[at:at + len(keys)]
        at += len(keys)
        assert np.array_equal(np.sort(want), np.arange(len(keys))), name
        assert np.all(np.diff(keys[want]) >= 0), name
        assert np.array_equal(fr.std_sort_perm(keys), want), name


def _straddle(rng, k, n, need):
    """len-n distances whose k-th smallest value tau = 10 is tied on both sides of row k: `need` of the
    rows >= k at tau enter the answer (0: rows < k at tau are themselves cut by std::sort's order)."""
    n_tail_below = k // 10
    n_head_tau = k // 3
    n_head_below = k - need - n_tail_below - n_head_tau + (7 if need == 0 else 0)
    head = np.concatenate([rng.integers(0, 10, n_head_below), np.full(n_head_tau, 10),
                           rng.integers(11, 21, k - n_head_below - n_head_tau)])
    tail = np.concatenate([rng.integers(0, 10, n_tail_below), np.full(3 * need + 20, 10)])
    tail = np.concatenate([tail, rng.integers(11, 21, n - k - tail.size)])
    return np.concatenate([rng.permutation(head), rng.permutation(tail)]).astype(np.int16)


def knn_reference_cases():
    """[(name, int16 distances, k)] for KNNFromDists with len >= k"""
    import stdsort_cases as sc
    rng = np.random.default_rng(77)
    cases = []
    for k in (64, 100, 1000, 1024):  # heads that take std::sort into its heap sort, then rows that displace them
        for g in (1, 5, k):
            head = sc.adversarial_keys(k) if g == 1 else sc.adversarial_tied(k, g)
            tail = rng.integers(0, int(head.max()) + 2, 700)
            cases.append((f"adversarial_k{k}_g{g}", np.concatenate([head, tail]).astype(np.int16), k))
    for k, n in ((100, 2000), (1000, 3000), (1024, 1024), (1024, 1025)):
        cases.append((f"all_equal_k{k}_n{n}", np.full(n, 321, np.int16), k))
    for k in (100, 1024):
        for need in (0, 1, 37):
            cases.append((f"straddle_k{k}_need{need}", _straddle(rng, k, k + 900, need), k))
    for k in (17, 100, 1024):
        d = rng.integers(0, 6, k + 1).astype(np.int16)
        cases.append((f"len_eq_k{k}", d[:k].copy(), k))
        for last in (0, 3, 9):  # the one row past k: below every other, tied, above
            d[k] = last
            cases.append((f"len_k_plus_1_k{k}_last{last}", d.copy(), k))
    return cases


def test_knn_from_dists_against_reference(oracle, request):
    """fast_ref.knn_from_dists against KNNFromDists<int16_t> compiled from the reference
    (oracle/ref_harness.cpp:ref_knn_from_dists; recorded under tests/golden/ref_tape/): heads that
    reach std::sort's heap-sort fallback, all-equal distances, ties at the cut on both sides of row k
    with none / one / many later rows entering, len = k and len = k + 1.  len < k is left out: the
    reference reads past its array there."""
    import stdsort_cases as sc
    from ref_tape import RefTape
    tape = RefTape(oracle, request.node.name)
    for name, d, k in knn_reference_cases():
        assert d.dtype == np.int16 and d.size >= k
        if name.startswith("adversarial"):
            assert sc.reaches_heap_sort(d[:k]), name
        if name.startswith("straddle"):
            tau = np.sort(d, kind="stable")[k - 1]
            assert (d[:k] == tau).any() and (d[k:] == tau).any(), name
        idx, dist = tape.call(lambda: oracle.ref_knn_from_dists(d, k), d, k)
        if name.startswith("straddle"):
            need = int(name.rsplit("need", 1)[1])
            assert int(((idx >= k) & (dist == tau)).sum()) == need, name
        lab, dis = fr.knn_from_dists(d, k)
        assert np.array_equal(lab, idx.astype(np.int64)), name
        assert np.array_equal(dis, dist.astype(np.float32)), name
