"""The integers of a best-first work unit (vaq_amd/csrc/vaq_scan_bf.h), restated in plain Python per layout policy.

A model of the kernel's arithmetic, not a reference for its output: what a round cuts a bucket into (units_of),
which rows a unit admits and which wave steps it loads (geometry), which of those steps need no row-range test
(interior_steps), how far the last step reads past the padded end of the rows (overread_rows) and how many rows of
slack the library allocates behind them (Policy.slack_rows).  tests/test_bf_unit_widths_cpu.py checks by brute force
that these tile every bucket and that the over-read never exceeds the slack; the same functions say what each case
of tests/test_bf_unit_widths.py plants.  Every function takes Python ints or numpy integer arrays.

The key rule (bucket_keys) is vaqhip_codes.cpp's build_rows and vaq_codes.hip's first_code_keys_kernel."""
import numpy as np

BF_SEG_STEPS = 64        # vaq_scan_bf.h:35, :62  (VAQ_BF_SEG: wave steps per work unit)
BF_MAX_BUCKETS = 1024    # vaq_scan_bf.h:67
BF_ROUND_BUCKETS = 128   # vaq_scan_bf.h:70, :72  (VAQ_BF_ROUND: buckets one round orders and scans)
TILE_ROWS = 64           # vaq_common.h
SCAN_MAX_THREADS = 1024  # vaq_scan.h  (SCAN_MAX_WAVES = 16, vaq_scan_params.h, times 64)


class Policy:
    """What scan_bf_body reads off its layout policy, and what the host pads and allocates for that layout."""

    def __init__(self, name, rows, align_rows, step_rows, slack_rows):
        self.name = name
        self.ROWS = rows                       # rows one lane holds per wave step (Pol::ROWS)
        self.WSTEP = 64 * rows                 # vaq_scan_bf.h:458  rows per wave step
        self.ALIGN_ROWS = align_rows           # Pol::ALIGN_ROWS: units start on a multiple of it (:460)
        self.SEG_ROWS = BF_SEG_STEPS * self.WSTEP  # vaq_scan_bf.h:459
        self.step_rows = step_rows             # scan_wg_step_rows(), vaq_scan_launch.hip
        self.slack_rows = slack_rows           # scan_bf_slack_words() / dwords per row, vaq_scan_bf.hip:48-54
        assert align_rows % rows == 0 and self.WSTEP % align_rows == 0  # vaq_scan_bf.h:278
        assert step_rows % self.WSTEP == 0

    def __repr__(self):
        return self.name

    def padded(self, N):
        """Rows the code array is padded to: build_rows / append_rows_bucketed, vaqhip_codes.cpp:21, :166."""
        return max(self.step_rows, -(-N // self.step_rows) * self.step_rows)

    @property
    def max_overread(self):
        """bf_overread_rows<Pol>(), vaq_scan_bf.h:1435."""
        return 64 * self.ROWS - self.ALIGN_ROWS


def bytes_policy(M):
    """BfBytes<M>, vaq_scan_bf.h:267-281."""
    item_bytes = 16 if M < 16 else M           # :268  (VAQ_BF_M8_ITEM_BYTES = 16, :247)
    rows = item_bytes // M                     # :251  BfBytesItem::ROWS
    align = 128 // M                           # :277  a 128-byte line
    step = SCAN_MAX_THREADS * (16 // M if M < 16 else 1)  # rows_per_item(), scan_wg_step_rows(), vaq_scan_launch.hip
    # vaq_scan_bf.hip:50: bf_overread_rows<BfBytes<M>>() * (M / 4) dwords, i.e. that many rows of M / 4 dwords
    return Policy(f"bytes{M}", rows, align, step, 64 * rows - align)


def bits_policy():
    """BfBits<W, CARRY>, vaq_scan_bf.h:351-357: a wave step is a tile, units start on tiles, no slack
    (vaq_scan_bf.hip:49)."""
    return Policy("bits", 1, TILE_ROWS, SCAN_MAX_THREADS, 0)


POLICIES = {8: bytes_policy(8), 16: bytes_policy(16), 32: bytes_policy(32), "bits": bits_policy()}


def clip(bs, be, r0, r1):
    """The rows of bucket [bs, be) inside the slice [r0, r1): vaq_scan_bf.h:643-644, :1131-1132."""
    return np.maximum(bs, r0), np.minimum(be, r1)


def units_of(pol, bs, be, r0, r1):
    """vaq_scan_bf.h:641-646.  (A bucket without rows in the slice gets the empty key, :626, and is never ordered:
    0 units.)"""
    s0, e0 = clip(bs, be, r0, r1)
    n = (e0 - (s0 & ~(pol.ALIGN_ROWS - 1)) + pol.SEG_ROWS - 1) // pol.SEG_ROWS
    return np.where(e0 > s0, n, 0) if isinstance(n, np.ndarray) else (int(n) if e0 > s0 else 0)


def geometry(pol, j, bs, be, r0, r1):
    """Unit j of the bucket: rows [pos, be), the row of its first item, its wave steps (vaq_scan_bf.h:1129-1141)."""
    s0, bend = clip(bs, be, r0, r1)
    al = s0 & ~(pol.ALIGN_ROWS - 1)                       # :1134
    pos = np.maximum(al + j * pol.SEG_ROWS, s0)           # :1135-1136
    e = np.minimum(al + (j + 1) * pol.SEG_ROWS, bend)     # :1137-1138
    base0 = pos & ~(pol.ALIGN_ROWS - 1)                   # :1139
    nst = (e - base0 + pol.WSTEP - 1) // pol.WSTEP        # :1140
    return pos, e, base0, nst


def interior_steps(pol, pos, be, base0, nst):
    """st_lo .. st_hi: the steps whose rows all lie in [pos, be) (vaq_scan_bf.h:1165-1168); the kernel tests the row
    range on the others only."""
    st_lo = np.where(pos > base0, 1, 0)
    st_hi = np.where(be < base0 + nst * pol.WSTEP, nst - 1, nst)
    return st_lo, st_hi


def overread_rows(pol, base0, nst, N):
    """Rows the unit's last step loads past the padded end of the rows (negative: it ends that far before it)."""
    return base0 + nst * pol.WSTEP - pol.padded(N)


def reaches_max_overread(pol, bs, N):
    """The two conditions under which the last unit of a bucket [bs, N) over-reads by pol.max_overread:
    its aligned start is congruent to WSTEP - ALIGN_ROWS modulo WSTEP, and N lies in the last ALIGN_ROWS rows below a
    multiple of the padded step or on that multiple."""
    al = bs & ~(pol.ALIGN_ROWS - 1)
    return (al % pol.WSTEP == pol.WSTEP - pol.ALIGN_ROWS) & (pol.padded(N) - N < pol.ALIGN_ROWS)


# ---- the key rule ---------------------------------------------------------------------------------------------
def key_shape(bucket_bits, bits0=8, bits1=8):
    """(shift, bt) of an index built with the bucket_bits option set (vaqhip_codes.cpp:39-53): the key is the top
    bucket_bits bits of the first code, continued -- once the whole first code is used -- by up to 4 top bits of the
    second."""
    kb = min(bucket_bits, bits0)
    shift = bits0 - kb
    bt = max(min(bucket_bits - kb, 4, bits1), 0) if shift == 0 else 0
    return shift, bt


def bucket_keys(codes, bucket_bits, bits0=8, bits1=8):
    """first_code_keys_kernel, vaq_codes.hip (without the fine bits, which order rows inside a bucket)."""
    shift, bt = key_shape(bucket_bits, bits0, bits1)
    key = codes[:, 0].astype(np.int64) >> shift
    if bt > 0:
        key = (key << bt) | (codes[:, 1].astype(np.int64) >> (bits1 - bt))
    return key, 1 << (bits0 - shift + bt)


def bucket_starts(codes, bucket_bits, bits0=8, bits1=8):
    """bucket_start[0 .. K0]: bucket b is rows [start[b], start[b + 1]) of the index's order (a stable sort by key;
    keys that do not occur are empty buckets, vaqhip_codes.cpp:84-86)."""
    key, K0 = bucket_keys(codes, bucket_bits, bits0, bits1)
    return np.concatenate([[0], np.cumsum(np.bincount(key, minlength=K0))]).astype(np.int64)


def default_key_bits(N):
    """Key bits build_rows picks when the option is unset (vaqhip_codes.cpp:13, :37-38), before the continuation."""
    want = 4
    while want < 10 and (2 << want) * 900 <= max(N, 1):
        want += 1
    return want


def slice_rows(pol, N, slices):
    """Rows per slice with the slices option set (vaqhip_plan.cpp:152-153)."""
    rows = -(-N // slices)
    return max(pol.step_rows, -(-rows // pol.step_rows) * pol.step_rows)


def bucket_units(pol, start, b, r0=0, r1=None):
    """[(pos, be, base0, nst)] of bucket b's units in the slice [r0, r1), as Python ints."""
    r1 = int(start[-1]) if r1 is None else r1
    bs, be = int(start[b]), int(start[b + 1])
    return [tuple(int(x) for x in geometry(pol, j, bs, be, r0, r1)) for j in range(units_of(pol, bs, be, r0, r1))]
