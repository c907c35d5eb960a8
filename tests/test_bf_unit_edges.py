"""Best-first scan (vaq_amd/csrc/vaq_scan_bf.h): the edges of a work unit and the admission of a wave step.

A unit of byte rows starts on a 128-byte line (Pol::ALIGN_ROWS: 16 rows of 8 bytes, 8 rows of 16), not on a whole
wave step; a wave step of two rows per lane admits its rows to the survivor queue one after the other.  The shapes
here put bucket starts on every residue that matters (0, 1, 15, 16, 17, 127 and an odd one modulo a wave step), make
buckets shorter than a line, exactly one wave step long, longer than a unit, cut by a slice and ending on the last
row of an array whose length is no multiple of 16; and they fill the queue not at all (k small, one row at distance
0) or completely (every row of the database survives its first group).

Reference: the CPU oracle.  Bar: distances bit for bit, labels under the tie contract of
helpers.assert_topk_matches; no tolerance.  Every search asserts that the best-first form served it."""
import numpy as np
import pytest

from helpers import assert_topk_matches

gpu = pytest.mark.gpu  # (per test: the shapes' own arithmetic below needs no GPU)

L = 4  # dimensions per subspace

# first-code buckets of the residue case: (first code, start row); the last one ends on row N - 1
STARTS = [(3, 0), (20, 129), (37, 271), (54, 400), (71, 528), (88, 657), (105, 895), (122, 902), (139, 1205),
          (255, 3158)]
N_RES = 3503


def test_residue_case_is_what_it_says():
    """The shapes' own arithmetic (no GPU): starts at the wanted residues modulo 128 and 16, the short bucket, the
    bucket of one wave step at residue 16, an array length that is no multiple of 16."""
    s = [x for _, x in STARTS]
    assert {x % 128 for x in s} >= {0, 1, 15, 16, 17, 127, 53}
    assert {x % 16 for x in s} >= {0, 1, 15}
    sizes = np.diff(s + [N_RES])
    assert sizes[6] == 7 and sizes[3] == 128 and s[3] % 128 == 16
    assert N_RES % 16 != 0 and N_RES % 128 != 0


def bucket_case(seed, M, starts, N, near=None, bits=8):
    """All-`bits`-bit index, unrotated.  Row r's first code is that of the bucket r falls into (rows are given in
    bucket order, shuffled before they are handed over).  One query per bucket, at that bucket's centroid of subspace
    0; the centroids of subspace 0 are ten times as far apart as the others', so a query's nearest rows are its own
    bucket's -- every row of a short bucket is in the answer, the rows at its edges included."""
    rng = np.random.default_rng(seed)
    cents = [(rng.normal(size=(1 << bits, L)) * (300.0 if s == 0 else 30.0)).astype(np.float32) for s in range(M)]
    codes = rng.integers(0, 1 << bits, size=(N, M), dtype=np.int64).astype(np.uint16)
    first = np.zeros(N, np.uint16)
    for (code, s), e in zip(starts, [x for _, x in starts[1:]] + [N]):
        first[s:e] = code
    codes[:, 0] = first
    codes = codes[rng.permutation(N)]
    qb = [c for c, _ in starts] if near is None else near
    X = (rng.normal(size=(len(qb), L * M)) * 30.0).astype(np.float32)
    for q, c in enumerate(qb):
        X[q, :L] = cents[0][c]
    return dict(bits=[bits] * M, cents=cents, X=X, codes=codes, eig=np.eye(L * M, dtype=np.float32))


_CASES = {}


def shared(oracle, name, make, ks):
    """A case and the oracle's answers for its ks: made once, shared by the tests that use it, never written to."""
    if name not in _CASES:
        c = make()
        nq, mb = c["X"].shape[0], max(c["bits"])
        ad = np.stack([oracle.all_dists(oracle.create_lut(c["X"][q], c["cents"], mb), c["codes"]) for q in range(nq)])
        want = {k: oracle.search(c["X"], c["cents"], c["codes"], k, max_bits=mb, projected=True) for k in ks}
        _CASES[name] = (c, ad, want)
    return _CASES[name]


def index_of(c, options):
    import vaq_amd
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(c["bits"])
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v._ensure_index()
    for key, val in options:  # (bucket_bits takes effect when the codes are set: first)
        v.set_option(key, val)
    v.mCodebook = c["codes"]
    return v


BF = (("queries_per_pass", 1), ("early_abandon", 1), ("best_first", 1), ("timing", 1))


def run(case, ks, what, options=(("bucket_bits", 8),), bf=1):
    """Every k through the best-first form (bf = 0: the shared-stream form) against the oracle.  Returns the answers
    and the last search's timing record."""
    c, ad, want = case
    nq = c["X"].shape[0]
    v = index_of(c, tuple(options) + tuple((k, (bf if k == "best_first" else x)) for k, x in BF))
    out, t = {}, None
    for k in ks:
        ans = v.search(c["X"], k)
        t = v.last_timing()
        assert t["best_first"] == bf, (what, k, t)
        lab, dis = ans.labels.reshape(nq, k).copy(), ans.distances.reshape(nq, k).copy()
        assert_topk_matches(lab, dis, want[k][0], want[k][1], ad, what=f"{what} k={k}")
        out[k] = (lab, dis)
    v.close()
    return out, t


def residues(oracle, M):
    return shared(oracle, f"residues{M}", lambda: bucket_case(5100 + M, M, STARTS, N_RES), (1, 2, 100, 256))


@gpu
def test_start_residues_and_sizes_m8(vaqlib, oracle):
    """8-byte rows: buckets starting at residues 0, 1, 15, 16, 17, 127, 6 and 53 modulo a wave step of 128 rows, one of
    7 rows, one of exactly 128 rows at residue 16, the last one ending on row N - 1 = 3502.  k = 256 takes in every
    row of the shorter buckets."""
    run(residues(oracle, 8), (100, 256), "residues M=8")


@gpu
def test_start_residues_m16(vaqlib, oracle):
    """16-byte rows (ALIGN_ROWS = 8, a wave step is 64 rows): the same starts."""
    run(residues(oracle, 16), (100, 256), "residues M=16")


@gpu
def test_few_survivors(vaqlib, oracle):
    """k = 1 and 2 with the query on a centroid of the dominant subspace: a tight threshold after the bootstrap, most
    wave steps admit nothing."""
    run(residues(oracle, 8), (1, 2), "few survivors")


@gpu
def test_two_slices_cut_a_bucket(vaqlib, oracle):
    """Two slices per query: rows [0, 2048) and [2048, 3503) -- r0 / r1 cut the bucket at rows [1205, 3158)."""
    _, t = run(residues(oracle, 8), (100,), "two slices", options=(("bucket_bits", 8), ("slices", 2)))
    assert t["slices"] == 2, t


@gpu
def test_invariance_without_best_first(vaqlib, oracle):
    """The shared-stream form on the same index: the same labels and the same distances, bit for bit."""
    case = residues(oracle, 8)
    a, _ = run(case, (100, 256), "bf")
    b, _ = run(case, (100, 256), "no bf", bf=0)
    for k in a:
        assert np.array_equal(a[k][1].view(np.uint32), b[k][1].view(np.uint32)), k
        assert np.array_equal(a[k][0], b[k][0]), k


@gpu
def test_fewer_rows_than_a_wave_step(vaqlib, oracle):
    """N = 100 < 128 in five buckets: every unit is one edge step, and the array ends inside it."""
    starts = [(9, 0), (60, 1), (61, 18), (130, 35), (200, 99)]
    case = shared(oracle, "tiny", lambda: bucket_case(5200, 8, starts, 100), (10, 100))
    run(case, (10, 100), "N=100")


LONG_STARTS = [(5, 0), (90, 77), (91, 9077), (170, 9090), (250, 9500)]
N_LONG = 10007


def long_case(oracle):
    return shared(oracle, "long", lambda: bucket_case(5300, 8, LONG_STARTS, N_LONG), (100,))


@gpu
def test_bucket_longer_than_a_unit(vaqlib, oracle):
    """A bucket of 9000 rows from row 77 (residue 13 modulo 16): two units, the second from al + SEG_ROWS = 64 + 8192,
    its first items prefetched into the ring while the first unit's last steps run."""
    assert LONG_STARTS[1][1] % 16 != 0 and LONG_STARTS[2][1] - LONG_STARTS[1][1] > 8192
    run(long_case(oracle), (100,), "long bucket")


@gpu
def test_deferred_second_launch(vaqlib, oracle):
    """defer_units = 1: the first launch scans one unit per query (for the query at the 77-row bucket fewer than k
    rows, so buckets stay in reach); the rest goes to the second launch, whose units have the same geometry."""
    _, t = run(long_case(oracle), (100,), "deferred", options=(("bucket_bits", 8), ("defer_units", 1)))
    assert t["deferred_queries"] >= 1, t


@gpu
def test_bit_packed_geometry_unchanged(vaqlib, oracle):
    """Bit-packed rows (12, 10, 9, 8, 8, 7, 6, 4 bits) keep whole tiles of 64 rows as their unit of alignment."""
    def make():
        rng = np.random.default_rng(5400)
        bits = [12, 10, 9, 8, 8, 7, 6, 4]
        cents = [(rng.normal(size=(1 << b, L)) * 30.0).astype(np.float32) for b in bits]
        X = (rng.normal(size=(4, L * len(bits))) * 30.0).astype(np.float32)
        codes = np.stack([rng.integers(0, 1 << b, size=5003, dtype=np.int64) for b in bits], 1).astype(np.uint16)
        return dict(bits=bits, cents=cents, X=X, codes=codes, eig=np.eye(L * len(bits), dtype=np.float32))
    run(shared(oracle, "bits", make, (100, 1)), (100, 1), "bit-packed", options=())


@gpu
@pytest.mark.parametrize("variant", ["equal", "two_of_three"])
def test_every_row_survives(vaqlib, oracle, variant):
    """One bucket of 3001 rows.  equal: every row is the same row -- both rows of all 64 lanes survive the first
    group in every step, 128 entries pass through the queue per step, the count reaches 64 with each row, and the
    answer's ties are resolved by label.  two_of_three: every third row has another third code and a larger
    first-group sum, so that a step appends about 85 entries and the count reaches 64 at either row of a step, with
    every leftover from 0 to 63."""
    def make():
        c = bucket_case(5500, 8, [(17, 0)], 3001, near=[17, 17])
        c["codes"][:] = c["codes"][0]
        if variant == "two_of_three":
            lut2 = ((c["cents"][2] - c["X"][0, 2 * L:3 * L]) ** 2).sum(1)
            c["codes"][::3, 2] = int(np.argmax(lut2))
        c["X"][1] = c["X"][0]
        return c
    run(shared(oracle, "survive_" + variant, make, (100, 256)), (100, 256), "every row " + variant)
