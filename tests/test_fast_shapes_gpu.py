"""FAST on the GPU at the shapes and edges tests/test_fast_gpu.py does not reach, against the same
checker (tests/fast_ref.py) and as strictly: labels and distances with np.array_equal.

  * every scan instantiation: fast_scan_kernel<CW>, CW = ceil(M / 32) = 1..4 -- M = 96 and 128 need
    2-bit (or narrower) codes to fit the 256 code bits a row packs -- and step counts T = M / 4 that
    are not a multiple of 8 (the `t >= T` exit inside a code word);
  * rows around the 32-row padding and the 128-row workgroup step, N = k and N = k + 1, query counts
    around the 64-query tile;
  * saturated tables: every distance 255 M (the last histogram bin; 32 641 bins at M = 128);
  * heads (the first k rows) that take std::sort into its heap-sort fallback, with ties at the cut on
    both sides of row k;
  * the append and rebuild paths of the code image at CW = 3 and 4.
"""
import numpy as np
import pytest

import fast_ref as fr
import stdsort_cases as sc
from helpers import make_case
from test_fast_gpu import check, fast_index, spread_quant

pytestmark = pytest.mark.gpu

MIX12 = [2, 1] * 64  # 192 code bits

SHAPES = [  # name, bits, D
    ("m4b4", [4] * 4, 16), ("m12b4", [4] * 12, 24), ("m20b4", [4] * 20, 40), ("m36b4", [4] * 36, 72),
    ("m40b4", [4] * 40, 80), ("m64b4", [4] * 64, 128), ("m80b3", [3] * 80, 80), ("m96b2", [2] * 96, 96),
    ("m128b2", [2] * 128, 128), ("m128b12", MIX12, 256),
]

# N, k, nq: N on both sides of the row padding (32) and the workgroup step (128), N = k and k + 1 at
# k = 100 and 1024, nq on both sides of the query tile (64) and of two tiles
SWEEP = [
    (31, 16, 1), (32, 17, 63), (33, 1, 64), (127, 100, 65), (128, 1024, 129), (129, 16, 64),
    (100, 100, 63), (101, 100, 129), (1024, 1024, 64), (1025, 1024, 65), (5000, 100, 65), (5000, 1024, 1),
    (5000, 17, 129),
]


def test_code_words_cover_every_scan_instantiation():
    """what the shape list is for: CW = ceil(M / 32) takes 1, 2, 3 and 4, and T = M / 4 leaves a
    partial last code word in most of them"""
    cw = {name: (len(bits) // 4 + 7) // 8 for name, bits, _ in SHAPES}
    assert set(cw.values()) == {1, 2, 3, 4}
    assert cw["m96b2"] == 3 and cw["m128b2"] == 4 and cw["m128b12"] == 4
    assert sum((len(bits) // 4) % 8 != 0 for _, bits, _ in SHAPES) >= 6
    assert all(sum(bits) <= 256 and max(bits) <= 4 for _, bits, _ in SHAPES)


@pytest.mark.parametrize("name,bits,D", SHAPES, ids=[s[0] for s in SHAPES])
def test_shape_sweep(vaqlib, name, bits, D):
    nq_max = max(nq for _, _, nq in SWEEP)
    c = make_case(300 + len(bits), D, bits, 1, nq_max)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    rng = np.random.default_rng(len(bits))
    for N, k, nq in SWEEP:
        codes = np.stack([rng.integers(0, 1 << b, size=N) for b in bits], 1).astype(np.uint16)
        codes[rng.integers(0, N, N // 10)] = codes[rng.integers(0, N, N // 10)]  # exact ties
        v.mCodebook = codes
        check(v, dict(c, X=c["X"][:nq], codes=codes), k, lut[:nq], what=f"{name} N={N} k={k} nq={nq}")
    v.close()


@pytest.mark.parametrize("bits,D", [([4] * 8, 16), ([4] * 64, 128), ([2] * 128, 128)], ids=["m8", "m64", "m128"])
@pytest.mark.parametrize("mode", ["all", "half"])
def test_saturated_tables(vaqlib, bits, D, mode):
    """tables whose entries clamp at 255: every one of them (all distances 255 M, the histogram's last
    bin) or about half of them (the mass in the top bins)"""
    M = len(bits)
    c = make_case(400 + M, D, bits, 3000, 20, dup_frac=0.05)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    lo = lut.min(axis=(0, 2)).astype(np.float32)
    if mode == "all":
        off, scale = lo - np.float32(1), np.full(M, 1e6, np.float32)
    else:  # every column's median entry lands on 255: the upper half of its entries clamp
        med = np.median(lut[..., : 1 << max(bits)].transpose(1, 0, 2).reshape(M, -1), axis=1).astype(np.float32)
        off, scale = lo, (np.float32(255) / np.maximum(med - lo, np.float32(1e-3))).astype(np.float32)
    v.setLUTQuantization(off, scale)
    small = v.buildSmallLUT(c["X"])
    assert np.array_equal(small, fr.small_lut16(lut, off, scale))
    live = small[..., : 1 << max(bits)]
    if mode == "all":
        assert (live == 255).all()
        assert (fr.row_dists(small[0], c["codes"]) == 255 * M).all()
    else:
        assert 0.25 < (live == 255).mean() < 0.75
    for k in (16, 100, 1024):
        _, dis = check(v, c, k, lut, what=f"M={M} {mode} k={k}")
        if mode == "all":
            assert (dis == np.float32(255 * M)).all()
    v.close()


# ---------------------------------------------------------------------- chosen distances --
# Eight one-dimensional subspaces of 4 bits, no rotation, a zero query: centroid j at sqrt(j + 1/2) makes
# table entry j about j + 1/2.  Five subspaces are scaled by 15 (entry floor(15 j + 7.5) = 15 j + 7, also
# when the float entry is a few ulp off j + 1/2), the others by 1 (entry j): a row whose codes spell key
# = 15 a + b, a spread over the scaled subspaces and b in one of the others, is at distance key + 35.
PLACE = np.array([15] * 5 + [1] * 3, np.float32)


def chosen_index():
    cents = [np.sqrt(np.arange(16, dtype=np.float64) + 0.5).astype(np.float32).reshape(16, 1) for _ in range(8)]
    return dict(D=8, M=8, L=1, bits=[4] * 8, cents=cents, eig=None)


def codes_for_keys(keys):
    keys = np.asarray(keys, np.int64)
    assert keys.min() >= 0 and keys.max() < 15 * 75
    codes = np.zeros((keys.size, 8), np.uint16)
    a = keys // 15
    for s in range(5):
        d = np.minimum(a, 15)
        codes[:, s] = d
        a = a - d
    codes[:, 5] = keys % 15
    return codes


def tail_keys(rng, head, k, need, drop):
    """rows after the head: enough rows below tau (a key several head rows share) that `need` of the
    later rows at tau enter the answer, or, with need = 0, that `drop` of the head's rows at tau leave it"""
    srt = np.sort(head)
    tau = int(srt[(3 * k) // 5])
    head_below, head_at = int((head < tau).sum()), int((head == tau).sum())
    n_below = k - head_below - head_at - need + drop
    assert tau > 0 and n_below > 0 and head_at > drop
    tail = np.concatenate([rng.integers(0, tau, n_below), np.full(need + 20, tau),
                           rng.integers(tau + 1, tau + 40, 600)])
    return rng.permutation(tail), tau


@pytest.mark.parametrize("k", [64, 100, 1000, 1024])
def test_adversarial_head_reaches_the_heap_sort(vaqlib, k):
    """the first k rows are a sequence that drives std::sort (and vaq::stdsort::sort on the device) past
    its depth limit; rows at the cut distance lie on both sides of row k, where the selection takes them
    by two different paths (rows < k by their place in std::sort's output, later rows in row order)"""
    rng = np.random.default_rng(k)
    c = chosen_index()
    c["X"] = np.zeros((3, 8), np.float32)
    c["codes"] = codes_for_keys([0])
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(np.zeros(8, np.float32), PLACE)
    small = v.buildSmallLUT(c["X"])
    assert np.array_equal(small, fr.small_lut16(lut, v.mOffsets, v.mScale))
    variants = [("distinct", sc.adversarial_keys(k), 9, 0), ("fives, later rows enter", sc.adversarial_tied(k, 5), 9, 0),
                ("fives, head rows leave", sc.adversarial_tied(k, 5), 0, 2),
                ("one run, head rows leave", sc.adversarial_tied(k, k), 0, 7)]
    for what, head, need, drop in variants:
        tail, tau = tail_keys(rng, head, k, need, drop)
        codes = codes_for_keys(np.concatenate([head, tail]))
        dists = fr.row_dists(small[0], codes)
        assert sc.reaches_heap_sort(dists[:k]), (k, what)  # on the real tables' distances
        cut = np.sort(dists, kind="stable")[k - 1]
        if "distinct" not in what:
            assert (dists[:k] == cut).any() and (dists[k:] == cut).any(), (k, what)
        v.mCodebook = codes
        lab, dis = check(v, dict(c, codes=codes), k, lut, what=f"k={k} {what}")
        if "distinct" not in what:
            assert int(((lab[0] >= k) & (dis[0] == cut)).sum()) == need, (k, what)
            assert int(((lab[0] < k) & (dis[0] == cut)).sum()) == int((dists[:k] == cut).sum()) - drop, (k, what)
        # N = k: the head alone
        v.mCodebook = codes[:k].copy()
        check(v, dict(c, codes=codes[:k]), k, lut, what=f"k={k} {what}, N = k")
    v.close()


# ------------------------------------------------------------------------------- paths --
@pytest.mark.parametrize("bits,D", [([2] * 96, 96), ([2] * 128, 128), (MIX12, 128)], ids=["cw3", "cw4", "cw4mix"])
def test_wide_rows_through_append_rebuild_and_device_entry(vaqlib, bits, D):
    """CW = 3 and 4 through the pack kernel for appended rows, the image rebuilt from the packed codes
    after a method switch, and the device-resident entry point"""
    import torch
    from vaq_amd import NNMethod
    c = make_case(500 + len(bits), D, bits, 3001, 70, dup_frac=0.05)
    v = fast_index(c)
    lut = v.build_lut(c["X"])
    v.setLUTQuantization(*spread_quant(lut))
    check(v, c, 100, lut, what="set_codes")
    extra = make_case(501, D, bits, 1500, 1)["codes"]
    v.add_codes(extra)                       # FAST in force: the new rows are packed behind the image
    c2 = dict(c, codes=np.concatenate([c["codes"], extra]))
    el, ed = check(v, c2, 100, lut, what="after add_codes")
    check(v, c2, 1024, lut, what="after add_codes, k = 1024")
    lab, dis = v.search_device(torch.from_numpy(c["X"]).cuda(), 100)
    torch.cuda.synchronize()
    assert np.array_equal(lab.cpu().numpy(), el) and np.array_equal(dis.cpu().numpy(), ed)
    v.mMethods = NNMethod.Heap
    v.search(c["X"], 10)                     # the image is released
    more = make_case(502, D, bits, 700, 1)["codes"]
    v.add_codes(more)                        # appended while HEAP is in force: no image to extend
    c3 = dict(c2, codes=np.concatenate([c2["codes"], more]))
    v.mMethods = NNMethod.Fast
    check(v, c3, 100, lut, what="image rebuilt from the packed codes")
    check(v, c3, 17, lut, what="image rebuilt, k = 17")
    v.close()
