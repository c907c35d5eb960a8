"""The unit arithmetic of the best-first scan (tests/bf_units_ref.py, restated from vaq_amd/csrc/vaq_scan_bf.h),
checked by brute force without a GPU, for 8-, 16- and 32-byte rows and the bit-packed policy:

  * the units of a bucket tile it -- disjoint, their union the bucket's rows inside the slice, as many as units_of
    says -- for every start residue, every length around one, two and SEG_ROWS / WSTEP wave steps and every cut;
  * a unit's first item is aligned, its first row lies in its first step, its last row in its last;
  * the last step of a unit reads at most 64 ROWS - ALIGN_ROWS rows past the padded end of the rows, exactly that
    many under two conditions and only then, and never more than the slack the library allocates;
  * every case of tests/test_bf_unit_widths.py plants what its docstring says.

The slack is not readable through an exported entry (scan_bf_slack_words is internal to the library): the bound is
compared with the restated bf_overread_rows, and test_restated_constants_match_the_sources pins the restatement to
the text of the sources."""
import os
import re

import numpy as np
import pytest

import bf_units_ref as U
import test_bf_unit_widths as W
from test_bf_unit_edges import L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLS = list(U.POLICIES.values())


def test_restated_constants_match_the_sources():
    csrc = os.path.join(ROOT, "vaq_amd", "csrc")
    h = open(os.path.join(csrc, "vaq_scan_bf.h")).read()
    hip = open(os.path.join(csrc, "vaq_scan_bf.hip")).read()
    k = open(os.path.join(csrc, "vaq_scan_launch.hip")).read()
    for text, pat in ((h, r"#define VAQ_BF_SEG %d\b" % U.BF_SEG_STEPS), (h, r"#define VAQ_BF_ROUND %d\b" % U.BF_ROUND_BUCKETS),
                      (h, r"constexpr int BF_MAX_BUCKETS = %d;" % U.BF_MAX_BUCKETS),
                      (h, r"#define VAQ_BF_M8_ITEM_BYTES 16\b"),
                      (h, r"BfBytesItem<M, \(M == 8 \? VAQ_BF_M8_ITEM_BYTES : \(M < 16 \? 16 : M\)\)> Item;"),
                      (h, r"static constexpr int ALIGN_ROWS = 128 / M;"),
                      (h, r"static constexpr int ALIGN_ROWS = TILE_ROWS;"),
                      (h, r"constexpr int WSTEP = 64 \* ROWS;"), (h, r"constexpr int SEG_ROWS = BF_SEG_STEPS \* WSTEP;"),
                      (h, r"bf_overread_rows\(\) \{ return 64 \* Pol::ROWS - Pol::ALIGN_ROWS; \}"),
                      (hip, r"if \(layout != LAYOUT_BYTES\) return 0;"),
                      (hip, r"return \(int64_t\)bf_overread_rows<BfBytes<A>>\(\) \* \(A / 4\);"),
                      (hip, r"#define VAQ_BF_BYTE_WIDTHS\(X\) X\(8\) X\(16\) X\(32\)"),
                      (k, r"\(layout == LAYOUT_BYTES && M < 16\) \? 16 / M : 1;"),
                      (k, r"return SCAN_MAX_THREADS \* rows_per_item\(layout, M\);")):
        assert re.search(pat, text), pat
    assert [(p.ROWS, p.WSTEP, p.ALIGN_ROWS, p.SEG_ROWS, p.step_rows, p.slack_rows) for p in POLS] == [
        (2, 128, 16, 8192, 2048, 112), (1, 64, 8, 4096, 1024, 56), (1, 64, 4, 4096, 1024, 60), (1, 64, 64, 4096, 1024, 0)]


# ---- the sweep --------------------------------------------------------------------------------------------------
def lengths(pol):
    return list(range(1, 2 * pol.WSTEP + 2)) + list(range(pol.SEG_ROWS - pol.WSTEP - 1, pol.SEG_ROWS + pol.WSTEP + 2))


def clipped_pairs(pol):
    """Every bucket [bs, be) with bs over two wave steps of residues and the lengths above, cut by every slice
    [r0, r1) that intersects it, reaches the scan as [max(bs, r0), min(be, r1)) -- units_of and geometry read
    nothing else (test_cuts_reach_the_scan_clipped).  Those pairs are the sub-intervals of the swept buckets; this
    yields all of [0, T), T the end of the last and longest bucket: a superset.  One start at a time, the ends as
    an array.  Then, uncut, the lengths around two units' rows, where a bucket has three."""
    T = 2 * pol.WSTEP - 1 + max(lengths(pol))
    far = 2 * pol.WSTEP + 2 * pol.SEG_ROWS + pol.WSTEP + 2  # (past every end: r1 cuts nothing)
    for s0 in range(T):
        yield s0, np.arange(s0 + 1, T + 1, dtype=np.int64), far
    for s0 in range(2 * pol.WSTEP):
        yield s0, s0 + np.arange(2 * pol.SEG_ROWS - pol.WSTEP - 1, 2 * pol.SEG_ROWS + pol.WSTEP + 2, dtype=np.int64), far


def test_cuts_reach_the_scan_clipped():
    """Real (bs, be, r0, r1), cuts outside, across and inside the bucket: the units are those of the clipped bucket,
    row for row; no intersection, no unit."""
    for pol in POLS:
        for bs in (0, 1, pol.ALIGN_ROWS - 1, pol.ALIGN_ROWS + 1, pol.WSTEP - 1):
            for n in (1, 3, pol.ALIGN_ROWS, pol.WSTEP + 2):
                be = bs + n
                for r0 in range(max(bs - 2, 0), be + 3):
                    for r1 in range(r0, be + 4):
                        s0, e0 = max(bs, r0), min(be, r1)
                        units = U.units_of(pol, bs, be, r0, r1)
                        if e0 <= s0:
                            assert units == 0
                            continue
                        assert units == U.units_of(pol, s0, e0, 0, e0) >= 1
                        rows = []
                        for j in range(units):
                            g = U.geometry(pol, j, bs, be, r0, r1)
                            assert g == U.geometry(pol, j, s0, e0, 0, e0)
                            rows += list(range(int(g[0]), int(g[1])))
                        assert rows == list(range(s0, e0)), (pol, bs, be, r0, r1)


@pytest.mark.parametrize("pol", POLS, ids=repr)
def test_units_tile_the_bucket(pol):
    """Unit 0 starts on the bucket's first row, unit j + 1 where unit j ends, the last one ends on the bucket's
    last row, each has rows; units_of counts them (the units past it are empty)."""
    longest = 0
    for s0, e0, T in clipped_pairs(pol):
        n = U.units_of(pol, s0, e0, 0, T)
        assert n.min() >= 1
        longest = max(longest, int(n.max()))
        at = np.full_like(e0, s0)
        for j in range(int(n.max()) + 2):
            pos, be = np.broadcast_arrays(*U.geometry(pol, j, s0, e0, 0, T)[:2])
            live = j < n
            assert np.all(be[~live] <= pos[~live]), (pol, s0, j)
            assert np.all(pos[live] == at[live]) and np.all(be[live] > pos[live]), (pol, s0, j)
            at = np.where(live, be, at)
        assert np.array_equal(at, e0), (pol, s0)
    assert longest == 3


@pytest.mark.parametrize("pol", POLS, ids=repr)
def test_items_stay_aligned_and_steps_in_range(pol):
    A, WS = pol.ALIGN_ROWS, pol.WSTEP
    for s0, e0, T in clipped_pairs(pol):
        n = U.units_of(pol, s0, e0, 0, T)
        for j in range(int(n.max())):
            live = j < n
            pos, be, base0, nst = (x[live] for x in np.broadcast_arrays(*U.geometry(pol, j, s0, e0, 0, T)))
            assert np.all(base0 % A == 0)
            assert np.all((base0 <= pos) & (pos < base0 + WS))
            assert np.all(((nst - 1) * WS < be - base0) & (be - base0 <= nst * WS))
            # the steps without a row-range test hold rows of the unit only, and only the first and the last step
            # are ever tested -- each exactly when rows outside the unit lie in it
            st_lo, st_hi = U.interior_steps(pol, pos, be, base0, nst)
            assert np.all((st_lo == 0) == (pos == base0)) and np.all((st_lo == 0) | (st_lo == 1))
            assert np.all((st_hi == nst) == (be == base0 + nst * WS)) and np.all((st_hi == nst) | (st_hi == nst - 1))
            some = st_hi > st_lo
            assert np.all((base0 + st_lo * WS >= pos)[some]) and np.all((base0 + st_hi * WS <= be)[some])


@pytest.mark.parametrize("pol", POLS, ids=repr)
def test_overread_bound_is_tight_and_covered(pol):
    """Every N of two padded steps -- from row 1, and again above two units' rows, where the last bucket has up to
    three units -- and every last bucket [bs, N): the last step of its last unit ends at most 64 ROWS - ALIGN_ROWS
    rows past the padded end (112 / 56 / 60 / 0), that many exactly when reaches_max_overread says so, never more
    than the slack; the units before the last end inside the rows.

    Why the bound holds: base0 is a multiple of ALIGN_ROWS and base0 + nst WSTEP < be + WSTEP, so the end of the
    last step is the largest number below be + WSTEP that is congruent to base0 modulo WSTEP; be <= N <= padded, a
    multiple of WSTEP, leaves it at most padded + WSTEP - ALIGN_ROWS.  (A unit that a slice cut ends stops short of
    the next slice's first WSTEP rows, which exist.)"""
    step = pol.step_rows
    above = -(-2 * pol.SEG_ROWS // step) * step
    worst, units_seen = -1 << 30, set()
    for lo in (0, above):
        for N in range(lo + 1, lo + 2 * step + 1):
            bs = np.arange(0, N, dtype=np.int64)
            n = U.units_of(pol, bs, N, 0, N)
            units_seen.update(np.unique(n).tolist())
            over = np.full_like(bs, -1 << 30)
            for j in range(int(n.max())):
                pos, be, base0, nst = U.geometry(pol, j, bs, N, 0, N)
                o = U.overread_rows(pol, base0, nst, N)
                last = j == n - 1
                assert np.all(o[j < n - 1] <= 0)
                over = np.where(last, o, over)
            assert np.all(over <= pol.slack_rows) and np.all(over <= pol.max_overread), (pol, N)
            assert np.array_equal(over == pol.max_overread, U.reaches_max_overread(pol, bs, N)), (pol, N)
            worst = max(worst, int(over.max()))
    assert worst == pol.max_overread == 64 * pol.ROWS - pol.ALIGN_ROWS == pol.slack_rows
    assert units_seen == {1, 2, 3}


# ---- the GPU cases ------------------------------------------------------------------------------------------------
_BUILT = {}


def built(name):
    if name not in _BUILT:
        _BUILT[name] = W.CASES[name][0]()
    return _BUILT[name]


def layout(name, bucket_bits):
    """(policy, bucket_start, populated buckets) of the case under the key rule."""
    c = built(name)
    pol = U.POLICIES[W.CASES[name][1]]
    start = U.bucket_starts(c["codes"], bucket_bits)
    assert c["codes"].shape[1] == W.CASES[name][1] and start[-1] == c["codes"].shape[0] <= 10_000
    assert 3 <= c["X"].shape[0] <= 10 or (name.startswith("overread") and c["X"].shape[0] == 2)
    return pol, start, np.nonzero(np.diff(start) > 0)[0]


def test_every_case_is_listed():
    assert sorted(W.CASES) == sorted(
        ["residues32", "long16", "long32", "long32x3", "coarse8", "coarse32"]
        + [f"overread{M}_{w}" for M in (8, 16, 32) for w in ("on", "below")]
        + [f"{n}{M}" for n in ("continued", "overflow") for M in (8, 16, 32)])
    for name, (_, M, bits) in W.CASES.items():
        for b in bits:  # which instantiation serves it: UL0 = (bucket_shift == 0), vaq_scan_bf.hip:69-71
            shift, bt = U.key_shape(b)
            assert (shift == 0) == (not name.startswith("coarse")) and (bt > 0) == name.startswith("continued")
            assert 16 <= 1 << (8 - shift + bt) <= U.BF_MAX_BUCKETS  # scan_bf_supported, vaq_scan_bf.hip:65


def check_residue_case(pol, start, pop, starts, N, wanted, short, one_step):
    assert [int(start[b]) for b in pop] == [s for _, s in starts] and start[-1] == N
    s = start[pop]
    assert {int(x) % pol.WSTEP for x in s} >= wanted and any(int(x) % pol.WSTEP % 2 for x in s)
    assert {int(x) % pol.ALIGN_ROWS for x in s} >= {0, 1, pol.ALIGN_ROWS - 1}
    sizes = np.diff(np.append(s, N))
    assert sizes[short[0]] == short[1] < pol.ALIGN_ROWS
    assert sizes[one_step[0]] == pol.WSTEP and s[one_step[0]] % pol.WSTEP == one_step[1]
    assert N % pol.ALIGN_ROWS != 0 and N % pol.WSTEP != 0 and start[pop[-1] + 1] == N


def test_residues32_is_what_it_says():
    pol, start, pop = layout("residues32", 8)
    check_residue_case(pol, start, pop, W.R32_STARTS, W.N_R32, {0, 1, 3, 4, 5, 60, 63}, (6, 3), (3, 4))
    # two slices: the cut lies inside a bucket, and both parts have rows
    cut = U.slice_rows(pol, W.N_R32, 2)
    assert cut == 2048 < W.N_R32 <= 2 * cut
    b = int(np.searchsorted(start, cut, side="right")) - 1
    assert start[b] < cut < start[b + 1]
    lo, hi = U.bucket_units(pol, start, b, 0, cut), U.bucket_units(pol, start, b, cut, W.N_R32)
    assert [(u[0], u[1]) for u in lo + hi] == [(int(start[b]), cut), (cut, int(start[b + 1]))]


@pytest.mark.parametrize("M", [8, 16, 32])
@pytest.mark.parametrize("where", ["on", "below"])
def test_overread_cases_reach_the_bound(M, where):
    pol, start, pop = layout(f"overread{M}_{where}", 8)
    N = int(start[-1])
    P = pol.padded(N)
    assert P == 2 * pol.step_rows and P - N == (0 if where == "on" else 2) and P - N < pol.ALIGN_ROWS
    last = int(pop[-1])
    bs = int(start[last])
    assert start[last + 1] == N and 300 <= N - bs <= 500 and bs % pol.ALIGN_ROWS != 0
    assert (bs & ~(pol.ALIGN_ROWS - 1)) % pol.WSTEP == pol.WSTEP - pol.ALIGN_ROWS
    units = U.bucket_units(pol, start, last)
    assert len(units) == 1
    assert U.overread_rows(pol, units[0][2], units[0][3], N) == pol.max_overread == pol.slack_rows
    assert bool(U.reaches_max_overread(pol, bs, N))
    c = built(f"overread{M}_{where}")  # a query on the last bucket's centroid, one on the first's
    assert np.array_equal(c["X"][0, :L], c["cents"][0][last]) and np.array_equal(c["X"][1, :L], c["cents"][0][pop[0]])


@pytest.mark.parametrize("name", list(W.LONG))
def test_long_cases_span_their_units(name):
    pol, start, pop = layout(name, 8)
    b = int(pop[1])
    bs, rows = int(start[b]), int(start[b + 1] - start[b])
    assert bs == 77 and bs % pol.ALIGN_ROWS != 0
    want = 3 if name == "long32x3" else 2
    assert rows == (2 * pol.SEG_ROWS + 70 if want == 3 else pol.SEG_ROWS + 500)
    units = U.bucket_units(pol, start, b)
    assert len(units) == want
    al = bs & ~(pol.ALIGN_ROWS - 1)
    assert [u[0] for u in units] == [bs] + [al + j * pol.SEG_ROWS for j in range(1, want)]
    assert start[pop[1]] - start[pop[0]] == 77 < 100  # the first bucket alone cannot fill k = 100: a unit is deferred


@pytest.mark.parametrize("M", [8, 32])
def test_coarse_cases_mix_first_codes(M):
    name = f"coarse{M}"
    c = built(name)
    starts, N = W.COARSE_STARTS[M]
    for bits in (4, 7):
        pol, start, pop = layout(name, bits)
        assert U.key_shape(bits) == (8 - bits, 0)
        assert [int(start[b]) for b in pop] == [s for _, s in starts] and start[-1] == N
        key, _ = U.bucket_keys(c["codes"], bits)
        first = c["codes"][np.argsort(key, kind="stable"), 0]  # first codes in the index's order
        lut0 = ((c["cents"][0][None, :, :] - c["X"][:, None, :L]) ** 2).sum(2)  # [query][code]
        for q, b in enumerate(pop):
            mine = first[start[b]:start[b + 1]]
            assert len(set(mine.tolist())) == 2 and np.all(mine[1:] != mine[:-1])  # alternating: every lane pair
            assert len(set(lut0[q, mine[:2]].tolist())) == 2  # ... and the two first terms differ for its query
    wanted = {0, 1, 15, 16, 17, 127, 53} if M == 8 else {0, 1, 3, 4, 5, 60, 63}
    assert {s % U.POLICIES[M].WSTEP for _, s in starts} >= wanted


@pytest.mark.parametrize("M", [8, 16, 32])
def test_continued_cases_pack_buckets_into_lines(M):
    name = f"continued{M}"
    c = built(name)
    for bits, bt in ((9, 1), (10, 2)):
        pol, start, pop = layout(name, bits)
        assert U.key_shape(bits) == (0, bt) and len(start) - 1 == 1 << bits
        sizes = np.diff(start)
        A = pol.ALIGN_ROWS
        bs, be = start[pop], start[pop + 1]
        assert (sizes[pop] < A).sum() >= 20  # buckets shorter than a line
        # a bucket that starts inside a line shares it with the one before: its unit loads that bucket's last rows
        # and must not admit them (starts are uniform modulo a line: (A - 1) / A of them, 3 in 4 at the least)
        assert (bs % A != 0).sum() >= len(pop) // 2
        # ... and a bucket wholly inside a line, with a neighbour on either side: three buckets in one line
        assert ((bs // A == (be - 1) // A) & (bs % A != 0) & (be % A != 0)).sum() >= 1
        # ... and units of neighbouring buckets load the same wave step
        b0, b1 = int(pop[0]), int(pop[1])
        u0, u1 = U.bucket_units(pol, start, b0)[0], U.bucket_units(pol, start, b1)[0]
        assert u1[2] < u0[2] + u0[3] * pol.WSTEP and u0[1] <= u1[0]
        # the queries: the first and the last bucket (which ends on row N - 1) among them
        key, _ = U.bucket_keys(c["codes"], bits)
        qkeys = []
        for q in range(c["X"].shape[0]):
            r = [r for r in range(len(key)) if np.array_equal(c["cents"][0][c["codes"][r, 0]], c["X"][q, :L])
                 and np.array_equal(c["cents"][1][c["codes"][r, 1]], c["X"][q, L:2 * L])]
            qkeys.append(int(key[r[0]]))
        assert int(pop[0]) in qkeys and int(pop[-1]) in qkeys and start[pop[-1] + 1] == W.N_CONT
    assert 1 << 10 == U.BF_MAX_BUCKETS and W.N_CONT % 64 != 0


@pytest.mark.parametrize("M", [8, 16, 32])
def test_overflow_cases_exceed_a_round(M):
    """200 populated buckets, each with a bound far below any k-th distance (the flat first table): all of them are
    eligible at once, against BF_ROUND_BUCKETS = 128.  Without bucket_bits = 8 the same rows make 16 buckets."""
    pol, start, pop = layout(f"overflow{M}", 8)
    c = built(f"overflow{M}")
    assert len(pop) == W.OVERFLOW_BUCKETS > U.BF_ROUND_BUCKETS
    lut0 = ((c["cents"][0][None, :, :] - c["X"][:, None, :L]) ** 2).sum(2)
    assert lut0[:, pop].max() < 320.0
    rest = sum(((c["cents"][s][c["codes"][:, s]][None] - c["X"][:, None, s * L:(s + 1) * L]) ** 2).sum(2)
               for s in range(1, M))  # [query][row]: what the other subspaces add
    assert np.sort(rest, axis=1)[:, 99].min() > 10 * 320.0  # the 100th smallest distance is far above every bound
    assert U.default_key_bits(c["codes"].shape[0]) == 4
    assert len(np.unique(U.bucket_keys(c["codes"], 4)[0])) <= 16 < U.BF_ROUND_BUCKETS


@pytest.mark.parametrize("M", [8, 32])
@pytest.mark.parametrize("where", ["on", "below"])
def test_appended_cases_move_every_bucket_start(M, where):
    """The first half of the rows is an index of other bucket starts; the merged one has the starts -- and the last
    unit's over-read -- of the index built at once."""
    c = built(f"overread{M}_{where}")
    N = c["codes"].shape[0]
    full = U.bucket_starts(c["codes"], 8)
    half, rest = U.bucket_starts(c["codes"][:N // 2], 8), U.bucket_starts(c["codes"][N // 2:], 8)
    assert np.array_equal(half + rest, full)  # append_rows_bucketed: tot_start = old_start + new_start
    pop = np.nonzero(np.diff(full) > 0)[0]
    assert np.all(half[pop[1:]] != full[pop[1:]]) and np.all(np.diff(half)[pop] > 0) and np.all(np.diff(rest)[pop] > 0)
    assert N < 4 * 4096  # merged in place, not rebuilt (add_codes_common, vaqhip_codes.cpp:210)
