"""The row packing the scan kernels assume, restated in numpy for the case table of
tests/test_scan_widths_gpu.py (no GPU needed).

LAYOUT_BITS (vaq_codes.hip, pack_codes_kernel): field s of a row occupies bits [bit_off, bit_off + bits)
of a W-dword little-endian row, LSB first; rows lie in planar tiles of 64 (vaq_common.h TILE_ROWS): word w
of row r at (r / 64) * 64 * W + w * 64 + r % 64.  The kernels take a field out of (lo, hi) = words
(word, word + 1) with a funnel shift by bit_off % 32 and a mask, and read hi as 0 when word is the row's
last (vaq_scan.h drain / tail_inplace, vaq_scan_bf.h BfBits::chain).  The best-first form keeps one packed
descriptor per subspace, word | shift << 3 | bits << 8 | lut_off << 12."""
import numpy as np
import pytest

from test_scan_widths_gpu import CASES, LDS_LIMIT, lut_floats, width

TILE_ROWS = 64
# allocations beyond the GPU table, for the descriptor arithmetic only: 15-bit fields, in word 7 too
EXTRA = {
    "w8_15bit": [15] * 16 + [4] * 4,      # 256 bits: 15-bit fields across every boundary
    "w1_15bit": [15, 1, 8, 8],
    "w8_last15": [8] * 26 + [6, 15, 8, 8, 8, 3],  # a 15-bit field straddling into word 7
}
ALL = dict({n: c[0] for n, c in CASES.items()}, **EXTRA)


def sub_desc(bits):
    """vaqhip_index_create_ex: (word, shift, bits, lut_off) per subspace."""
    out, bit_off, lut_off = [], 0, 0
    for b in bits:
        out.append((bit_off // 32, bit_off % 32, b, lut_off))
        bit_off += b
        lut_off += 1 << b
    return out


def first_sub(bits):
    """first_sub[w] = the first subspace whose field starts at or after bit 32 * w (M when none)."""
    W, M = width(bits), len(bits)
    offs = np.concatenate([[0], np.cumsum(bits)[:-1]])
    return [next((s for s in range(M) if offs[s] >= 32 * w), M) for w in range(W + 1)]


def pack(codes, bits):
    """uint16 [N, M] -> planar tiles uint32 [ceil(N / 64), W, 64], rows past N zero."""
    N, W = codes.shape[0], width(bits)
    rows = np.zeros((-(-N // TILE_ROWS) * TILE_ROWS, W), np.uint32)
    for s, (word, shift, b, _) in enumerate(sub_desc(bits)):
        v = codes[:, s].astype(np.uint64) << np.uint64(shift)
        rows[:N, word] |= (v & np.uint64(0xffffffff)).astype(np.uint32)
        if shift + b > 32:
            rows[:N, word + 1] |= (v >> np.uint64(32)).astype(np.uint32)
    return np.ascontiguousarray(rows.reshape(-1, TILE_ROWS, W).transpose(0, 2, 1))


def word_of(tiles, r, w):
    return tiles[r // TILE_ROWS, w, r % TILE_ROWS]


def decode(tiles, bits, N, hi_zero_at=None):
    """What the kernels read: alignbit(hi, lo, shift) & mask with hi = 0 past the last word.
    hi_zero_at = w: the same with hi forced to 0 for fields of word w (a broken kernel)."""
    W = width(bits)
    r = np.arange(N)
    out = np.empty((N, len(bits)), np.uint16)
    for s, (word, shift, b, _) in enumerate(sub_desc(bits)):
        lo = word_of(tiles, r, word).astype(np.uint64)
        hi = word_of(tiles, r, word + 1).astype(np.uint64) if word + 1 < W else np.zeros(N, np.uint64)
        if hi_zero_at == word:
            hi = np.zeros(N, np.uint64)
        funnel = ((hi << np.uint64(32)) | lo) >> np.uint64(shift)
        out[:, s] = (funnel & np.uint64(0xffffffff) & np.uint64((1 << b) - 1)).astype(np.uint16)
    return out


def random_codes(bits, N, seed):
    rng = np.random.default_rng(seed)
    codes = np.stack([rng.integers(0, 1 << b, size=N) for b in bits], 1).astype(np.uint16)
    codes[0] = [(1 << b) - 1 for b in bits]  # every bit of the row set
    codes[1] = 0
    return codes


@pytest.mark.parametrize("name", list(ALL))
def test_fields_come_back_by_funnel_shift_and_mask(name):
    bits = ALL[name]
    N = 131  # two tiles and three rows: the last tile is ragged
    codes = random_codes(bits, N, 17)
    tiles = pack(codes, bits)
    W = width(bits)
    assert tiles.shape == (3, W, TILE_ROWS) and not tiles[2, :, 3:].any()
    # the flat index the kernels use
    flat = tiles.ravel()
    for r in (0, 63, 64, 130):
        for w in range(W):
            assert flat[(r // 64) * 64 * W + w * 64 + r % 64] == word_of(tiles, r, w)
    assert np.array_equal(decode(tiles, bits, N), codes)
    # row 0 has every code bit set: exactly sum(bits) bits of the row are
    ones = sum(bin(int(word_of(tiles, 0, w))).count("1") for w in range(W))
    assert ones == sum(bits)
    # every dword carries bits of some field, and no field needs a word past the row
    for word, shift, b, _ in sub_desc(bits):
        assert word < W and (shift + b <= 32 or word + 1 < W)


@pytest.mark.parametrize("name", list(ALL))
def test_hi_is_zero_exactly_for_fields_of_the_last_word(name):
    """`hi = cur_word + 1 < W ? ... : 0`: taken for the fields that start in the last dword, which never
    reach past it; a field that straddles always has a next word to read."""
    bits = ALL[name]
    W = width(bits)
    sd = sub_desc(bits)
    last = [s for s, d in enumerate(sd) if d[0] == W - 1]
    for s, (word, shift, b, _) in enumerate(sd):
        if s in last:
            assert shift + b <= 32, (name, s)
        elif shift + b > 32:
            assert word + 1 < W, (name, s)
    fs = first_sub(bits)
    assert fs[0] == 0 and fs[W] == len(bits) and all(fs[w] <= fs[w + 1] for w in range(W))
    assert last == list(range(fs[W - 1], len(bits)))


def test_both_sides_of_the_last_word_branch_are_in_the_table():
    """Rows that fill the last dword have fields starting in it (hi = 0 taken); the 161-bit row has a
    single bit there, reached only as the hi half of a field of dword 4 (the branch is never taken)."""
    for name in ("w5_bytes20", "w6_full", "w7_full", "w8_m128", "w4_bf"):
        bits = ALL[name]
        assert sum(bits) % 32 == 0 and any(d[0] == width(bits) - 1 for d in sub_desc(bits)), name
    bits = ALL["w6_ragged"]
    sd = sub_desc(bits)
    assert not any(d[0] == 5 for d in sd)
    assert [s for s, d in enumerate(sd) if d[0] == 4 and d[1] + d[2] > 32] == [len(bits) - 1]
    bits = ALL["w8_resident"]
    assert sub_desc(bits)[-1][:3] == (7, 24, 1)  # the 1-bit field is decoded from word 7


def straddlers(bits, w):
    return [s for s, d in enumerate(sub_desc(bits)) if d[0] == w and d[1] + d[2] > 32]


@pytest.mark.parametrize("w", range(7))
def test_a_decode_broken_at_one_word_changes_the_cases_that_straddle_it(w):
    """Force hi = 0 for the fields of dword w, as a broken drain / chain would: the decoded codes (hence
    the distances the GPU file compares bit for bit) change for exactly the cases with a field across
    the boundary w / w + 1.  Every boundary from 3 / 4 up is crossed by a field of subspace >= 4 in some
    case of the GPU table, for W = 5, 6, 7 and 8 each."""
    hit = set()
    for name, (bits, _, _) in CASES.items():
        if w >= width(bits):
            continue
        codes = random_codes(bits, 131, 23)
        tiles = pack(codes, bits)
        broken = decode(tiles, bits, 131, hi_zero_at=w)
        cols = np.nonzero((broken != codes).any(0))[0].tolist()
        assert cols == straddlers(bits, w), (name, w)
        if cols:
            hit.add(name)
    assert hit == {n for n, (b, _, _) in CASES.items() if straddlers(b, w)}
    for wd in range(w + 2, 9) if w >= 3 else ():
        assert any(width(CASES[n][0]) == wd and max(straddlers(CASES[n][0], w)) >= 4 for n in hit), (w, wd)
    if w == 4:  # the example of the kind: hi = 0 at dword 4 in drain
        assert hit == {"w6_ragged", "w6_full", "w6_tail", "w7_straddle", "w7_full", "w7_tail", "w8_straddle"}


@pytest.mark.parametrize("name", list(CASES))
def test_a_kernel_that_misses_one_dword_changes_every_case(name):
    """Dword w of the rows read as zero (a wrong tile stride, a wrong `first_sub[w]`): the codes of exactly
    the fields that touch it change, for every dword of every case -- also the byte-aligned ones, which no
    funnel shift can break."""
    bits = CASES[name][0]
    codes = random_codes(bits, 131, 29)
    tiles = pack(codes, bits)
    for w in range(width(bits)):
        blind = tiles.copy()
        blind[:, w, :] = 0
        cols = np.nonzero((decode(blind, bits, 131) != codes).any(0))[0].tolist()
        touch = [s for s, (word, shift, b, _) in enumerate(sub_desc(bits))
                 if word == w or (word + 1 == w and shift + b > 32)]
        assert cols == touch and touch, (name, w)


def pack_desc(word, shift, b, lut_off):
    d = word | (shift << 3) | (b << 8) | (lut_off << 12)
    assert d < 1 << 32
    return d


def unpack_desc(d):
    return d & 7, (d >> 3) & 31, (d >> 8) & 15, d >> 12


@pytest.mark.parametrize("name", list(ALL))
def test_best_first_descriptor_round_trips(name):
    bits = ALL[name]
    assert len(bits) <= 128  # VAQ_BF_MAX_SUBS descriptors
    for d in sub_desc(bits):
        assert unpack_desc(pack_desc(*d)) == d, (name, d)


def test_best_first_descriptor_limits():
    """Word 7, shift 31, 15 bits and the largest table offset LDS admits (the best-first form needs
    every table resident: fewer than 160 KiB / 4 entries) fit their fields; the fields do not overlap."""
    top = LDS_LIMIT // 4 - 1
    for d in [(7, 31, 15, top), (7, 0, 1, 0), (0, 31, 15, 0), (0, 0, 15, top), (7, 24, 1, 7936)]:
        assert unpack_desc(pack_desc(*d)) == d
    assert top < 1 << 20
    # in the table: word 7 is decoded, M = 128 fills the array, the largest offset is a tail case's
    assert any(d[0] == 7 for d in sub_desc(ALL["w8_resident"])) and len(ALL["w8_m128"]) == 128
    assert max(lut_floats(b) for b in ALL.values() if 4 * lut_floats(b) <= LDS_LIMIT) <= top + 1
    assert max(b for bits in EXTRA.values() for b in bits) == 15
    assert any(d[0] == 6 and d[1] + d[2] > 32 and d[2] == 15 for d in sub_desc(EXTRA["w8_last15"]))


def test_carry_form_needs_at_most_two_dwords():
    """scan_bits_bf_kernel<W, CARRY = true> is chosen when sub[4].word == W - 1 (vaqhip_plan.cpp): four
    fields of at most 15 bits end by bit 60, so sub[4].word <= 1 and the form is unreachable for W >= 3."""
    assert 4 * 15 // 32 == 1
    for name, bits in ALL.items():
        if len(bits) > 4 and width(bits) >= 3:
            assert sub_desc(bits)[4][0] <= 1 < width(bits) - 1, name
