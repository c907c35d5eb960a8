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
