"""Best-first scan (vaq_amd/csrc/vaq_scan_bf.h): the edges of a work unit for every byte width and key form.

tests/test_bf_unit_edges.py pins the unit geometry for 8-byte rows (partly 16) keyed by the whole first code.  Here:
32-byte rows (ALIGN_ROWS = 4, QCW = 0: the tail re-reads the row from the code array), keys coarser than the first
code (UL0 = false: the first term per row), keys continued into the second code (bt > 0: several buckets inside one
128-byte line), the largest over-read the slack behind the code array allows, buckets of two and three units at 16
and 32 bytes, more eligible buckets than a round holds, and rows that arrived through add_codes.

What each case plants -- start residues, the bucket shorter than a line, the one of exactly a wave step, the units a
bucket spans, the over-read of the last unit, the buckets per line, the bucket count -- is proven without a GPU in
tests/test_bf_unit_widths_cpu.py from the codes below, through tests/bf_units_ref.py.

Reference: the CPU oracle.  Bar: distances bit for bit, labels under the tie contract of
helpers.assert_topk_matches; no tolerance.  Every search asserts that the best-first form served it.

Kernel instantiation per case (scan_bytes_bf_kernel<M, UL0>; UL0 = the key is the whole first code or more):
residues32, overread32, long32, long32x3, overflow32, appended (M = 32), continued (M = 32): <32, true>;
overread16, long16, overflow16, continued (M = 16): <16, true>; overread8, overflow8, appended (M = 8), continued
(M = 8): <8, true>; coarse (bucket_bits 4 and 7): <8, false> and <32, false>."""
import numpy as np
import pytest

from bf_units_ref import POLICIES
from helpers import assert_topk_matches
from test_bf_serial_phases import flat_first_table_case
from test_bf_unit_edges import BF, L, STARTS, N_RES, bucket_case, index_of, run, shared

gpu = pytest.mark.gpu  # (per test: the cases themselves are built and checked without a GPU)

# ---- residues32: (first code, start row), modulo 64: 0, 1, 3, 4, 4, 5, 60, 63, 41, 24 -----------------------------
# [260, 324) is exactly one wave step from residue 4, [700, 703) is shorter than a line, the last bucket ends on row
# N - 1 = 3502; two slices cut at row 2048, inside [1001, 2200)
R32_STARTS = [(3, 0), (20, 65), (37, 195), (54, 260), (71, 324), (88, 453), (105, 700), (122, 703), (139, 1001),
              (255, 2200)]
N_R32 = 3503


def residues32_case():
    return bucket_case(6100, 32, R32_STARTS, N_R32)


# ---- overread: the last bucket's aligned start on residue WSTEP - ALIGN_ROWS, N on / two rows below a padded step --
OVER_OFFSET = {8: 5, 16: 3, 32: 1}  # the bucket's start inside its line


def overread_shape(M, below):
    """(starts, N): N = two padded steps (less 2 rows: still in the last ALIGN_ROWS rows); the last bucket starts
    384 + ALIGN_ROWS rows before the padded end, plus an offset inside the line: about 390 rows."""
    pol = POLICIES[M]
    P = 2 * pol.step_rows
    last = P - (384 + pol.ALIGN_ROWS) + OVER_OFFSET[M]
    return [(3, 0), (40, 300), (90, 777), (255, last)], P - (2 if below else 0)


def overread_case(M, below):
    starts, N = overread_shape(M, below)
    return bucket_case(6200 + M + (1 if below else 0), M, starts, N, near=[255, 3])


# ---- long: a bucket of SEG_ROWS + 500 rows (two units), one of 2 SEG_ROWS + 70 (three), from row 77 ---------------
def long_starts(rows):
    a = 77 + rows
    return [(5, 0), (90, 77), (91, a), (170, a + 13), (250, a + 423)], a + 930


LONG = {"long16": (16, 4096 + 500), "long32": (32, 4096 + 500), "long32x3": (32, 2 * 4096 + 70)}


def long_case(name):
    M, rows = LONG[name]
    starts, N = long_starts(rows)
    return bucket_case(6300 + M + rows % 7, M, starts, N)


# ---- coarse: bucket_bits 4 and 7, two first codes per bucket in alternation ---------------------------------------
COARSE_STARTS = {8: (STARTS, N_RES), 32: (R32_STARTS, N_R32)}


def coarse_case(M):
    """The buckets of the residue cases; row by row (in the order the rows are handed over, which is the order
    inside a bucket) a bucket's first code alternates between c and c ^ 1 -- one key at 7 key bits and at 4 -- whose
    centroids lie a few units apart: both kinds of row are among the query's nearest, and their first terms differ
    from lane to lane."""
    starts, N = COARSE_STARTS[M]
    c = bucket_case(6400 + M, M, starts, N)
    rng = np.random.default_rng(6450 + M)
    for code, _ in starts:
        rows = np.nonzero(c["codes"][:, 0] == code)[0]
        c["codes"][rows[1::2], 0] = code ^ 1
        c["cents"][0][code ^ 1] = c["cents"][0][code] + (rng.normal(size=L) * 3.0).astype(np.float32)
    return c


# ---- continued: bucket_bits 9 and 10, uniform codes: 512 / 1024 buckets of a few rows -----------------------------
N_CONT = 3503


def continued_case(M):
    """Uniform first and second codes.  The queries sit on the first two centroids of four rows: those of the
    smallest and of the largest 10-bit key (the first bucket, and the one that ends on row N - 1) and two others."""
    rng = np.random.default_rng(6500 + M)
    cents = [(rng.normal(size=(256, L)) * (300.0 if s == 0 else 30.0)).astype(np.float32) for s in range(M)]
    codes = rng.integers(0, 256, size=(N_CONT, M), dtype=np.int64).astype(np.uint16)
    key = codes[:, 0].astype(np.int64) * 4 + (codes[:, 1] >> 6)
    picks = [int(np.argmin(key)), int(np.argmax(key)), 1000, 2000]
    X = (rng.normal(size=(len(picks), L * M)) * 30.0).astype(np.float32)
    for q, r in enumerate(picks):
        X[q, :L] = cents[0][codes[r, 0]]
        X[q, L:2 * L] = cents[1][codes[r, 1]]
    return dict(bits=[8] * M, cents=cents, X=X, codes=codes, eig=np.eye(L * M, dtype=np.float32))


# ---- overflow: 200 populated buckets under a flat first table -----------------------------------------------------
OVERFLOW_BUCKETS = 200


def overflow_case(M):
    """test_bf_serial_phases.flat_first_table_case (8 subspaces) with 200 first codes, widened to M subspaces: the
    first table, and with it every bucket's bound, is that case's; the added terms only raise the distances."""
    c = flat_first_table_case(6600 + M, OVERFLOW_BUCKETS, nq=3)
    rng = np.random.default_rng(6650 + M)
    N, nq = c["codes"].shape[0], c["X"].shape[0]
    for _ in range(M - 8):
        c["cents"].append((rng.normal(size=(256, L)) * 30.0).astype(np.float32))
    c["X"] = np.hstack([c["X"], (rng.normal(size=(nq, L * (M - 8))) * 30.0).astype(np.float32)])
    c["codes"] = np.hstack([c["codes"], rng.integers(0, 256, size=(N, M - 8), dtype=np.int64).astype(np.uint16)])
    c["bits"] = [8] * M
    c["eig"] = np.eye(L * M, dtype=np.float32)
    return c


# Every case: name -> (builder, M, the bucket_bits it is searched with).  (The CPU test walks this table.)
CASES = {"residues32": (residues32_case, 32, (8,))}
for _M in (8, 16, 32):
    for _below in (False, True):
        CASES[f"overread{_M}_{'below' if _below else 'on'}"] = (
            lambda M=_M, below=_below: overread_case(M, below), _M, (8,))
for _name in LONG:
    CASES[_name] = (lambda name=_name: long_case(name), LONG[_name][0], (8,))
for _M in (8, 32):
    CASES[f"coarse{_M}"] = (lambda M=_M: coarse_case(M), _M, (4, 7))
for _M in (8, 16, 32):
    CASES[f"continued{_M}"] = (lambda M=_M: continued_case(M), _M, (9, 10))
    CASES[f"overflow{_M}"] = (lambda M=_M: overflow_case(M), _M, (8,))


def case(oracle, name, ks):
    return shared(oracle, "widths_" + name, CASES[name][0], ks)


# ---- residues32 ---------------------------------------------------------------------------------------------------
@gpu
def test_residues32(vaqlib, oracle):
    """32-byte rows: starts at residues 0, 1, 3, 4, 5, 60, 63, 41 and 24 modulo a wave step of 64 rows, a bucket of 3
    rows, one of exactly 64 at residue 4, the last one ending on row 3502.  Every survivor's tail is re-read from the
    code array by its row number (QCW = 0)."""
    run(case(oracle, "residues32", (100, 256)), (100, 256), "residues32")


@gpu
def test_residues32_two_slices(vaqlib, oracle):
    """Rows [0, 2048) and [2048, 3503): the cut falls inside the bucket at [1001, 2200)."""
    _, t = run(case(oracle, "residues32", (100, 256)), (100, 256), "residues32 slices",
               options=(("bucket_bits", 8), ("slices", 2)))
    assert t["slices"] == 2, t


@gpu
def test_residues32_without_best_first(vaqlib, oracle):
    """The shared-stream form on the same index: the same labels, the same distances bit for bit."""
    c = case(oracle, "residues32", (100, 256))
    a, _ = run(c, (100, 256), "residues32 bf")
    b, _ = run(c, (100, 256), "residues32 no bf", bf=0)
    for k in a:
        assert np.array_equal(a[k][1].view(np.uint32), b[k][1].view(np.uint32)), k
        assert np.array_equal(a[k][0], b[k][0]), k


# ---- overread -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("where", ["on", "below"])
@pytest.mark.parametrize("M", [8, 16, 32])
def test_overread(vaqlib, oracle, M, where):
    """The last unit's last step loads 64 ROWS - ALIGN_ROWS rows (112 / 56 / 60) past the padded end of the rows:
    all of the slack scan_bf_slack_words() adds and not a row more (test_bf_unit_widths_cpu proves both).  The rows
    read there belong to no unit; the last bucket's own last rows are in the answer."""
    name = f"overread{M}_{where}"
    run(case(oracle, name, (100,)), (100,), name)


# ---- long ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("name", list(LONG))
def test_long_bucket(vaqlib, oracle, name, defer):
    """A bucket of SEG_ROWS + 500 rows from row 77 (no multiple of ALIGN_ROWS): two units, the second from
    al + SEG_ROWS; 2 SEG_ROWS + 70 rows: three.  defer = 1: the first launch scans one unit per query, the second
    the rest (the query at the 77-row bucket has fewer than k rows after its first unit)."""
    opts = (("bucket_bits", 8),) + ((("defer_units", 1),) if defer else ())
    _, t = run(case(oracle, name, (100,)), (100,), f"{name} defer={defer}", options=opts)
    if defer:
        assert t["deferred_queries"] >= 1, t


# ---- coarse -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bucket_bits", [4, 7])
@pytest.mark.parametrize("M", [8, 32])
def test_coarse_keys(vaqlib, oracle, M, bucket_bits):
    """UL0 = false: the key is the top 4 or 7 bits of the first code, a bucket's rows carry two first codes in
    alternation and every row looks its own first term up."""
    name = f"coarse{M}"
    run(case(oracle, name, (100,)), (100,), f"{name} bits={bucket_bits}", options=(("bucket_bits", bucket_bits),))


# ---- continued ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bucket_bits", [9, 10])
@pytest.mark.parametrize("M", [8, 16, 32])
def test_continued_keys(vaqlib, oracle, M, bucket_bits):
    """bt = 1 and 2: 512 and 1024 (BF_MAX_BUCKETS) buckets of a few rows; neighbouring buckets share an aligned
    line, so neighbouring units load the same rows and each must admit its own only."""
    name = f"continued{M}"
    run(case(oracle, name, (10, 100)), (10, 100), f"{name} bits={bucket_bits}",
        options=(("bucket_bits", bucket_bits),))


# ---- overflow -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", [8, 16, 32])
def test_round_overflow(vaqlib, oracle, M):
    """200 eligible buckets against BF_ROUND_BUCKETS = 128: the bisection (Pol::BISECT_IN_PLACE), then a second
    round.  bucket_bits = 8 is what makes the buckets 200: left to itself an index of 6000 rows keys its rows by 4
    bits (16 buckets), so 8-byte rows are here as well."""
    name = f"overflow{M}"
    run(case(oracle, name, (100,)), (100,), name)


# ---- appended -----------------------------------------------------------------------------------------------------
ID_BASE = 1000


@gpu
@pytest.mark.parametrize("where", ["on", "below"])
@pytest.mark.parametrize("M", [8, 32])
def test_appended_rows(vaqlib, oracle, M, where):
    """The over-read shapes built from all rows at once and from the first half of the (shuffled) rows plus
    add_codes of the rest, which merges bucket by bucket into a new code array -- with its own slack -- and moves
    every bucket start.  Labels carry id_base.  Both against the oracle, and against each other exactly."""
    name = f"overread{M}_{where}"
    c, ad, want = case(oracle, name, (100,))
    nq, k = c["X"].shape[0], 100
    o_lab = np.where(want[k][0] >= 0, want[k][0] + ID_BASE, -1)
    N = c["codes"].shape[0]
    got = []
    for split in (N, N // 2):
        v = index_of(dict(c, codes=c["codes"][:split]), (("bucket_bits", 8),) + BF)
        v.id_base = ID_BASE
        if split < N:
            v.add_codes(c["codes"][split:])
        ans = v.search(c["X"], k)
        t = v.last_timing()
        assert t["best_first"] == 1, (name, split, t)
        lab, dis = ans.labels.reshape(nq, k).copy(), ans.distances.reshape(nq, k).copy()
        v.close()
        assert_topk_matches(lab, dis, o_lab, want[k][1], ad, id_base=ID_BASE, what=f"{name} split={split}")
        got.append((lab, dis))
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
    assert np.array_equal(got[0][0], got[1][0])
