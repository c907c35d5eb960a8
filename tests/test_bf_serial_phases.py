"""The serial phases of the best-first scan (vaq_amd/csrc/vaq_scan_bf.h) at the edges of their code: the
bootstrap's selection of the q-th smallest of a wave's 64 lane minima (wave_sort64), the ordering of a round's
buckets (eight keys per trip, a tail of one to seven), the final ranking, and the DPP prefix sums
(wave_prefix_incl) -- on shapes built to reach those edges rather than the benchmark's.

Reference: the CPU oracle.  Bar: distances bit for bit, labels under the tie contract of
helpers.assert_topk_matches; no tolerance.  The index has no stat that counts rounds, so the round tests
assert results only; every search asserts that the best-first form served it."""
import os
import subprocess

import numpy as np
import pytest

from helpers import assert_topk_matches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, M, L = 32, 8, 4
BF_RANK_SORT_MAX = 256  # vaq_scan_bf.h


def base_case(seed, bits, N, nq):
    """Unrotated index (identity eigenvectors: the projected query is the query).  Every query shares its first
    L coordinates, so all of them see the same first lookup table."""
    rng = np.random.default_rng(seed)
    m = len(bits)
    cents = [(rng.normal(size=(1 << b, L)) * 30.0).astype(np.float32) for b in bits]
    X = (rng.normal(size=(nq, L * m)) * 30.0).astype(np.float32)
    X[:, :L] = X[0, :L]
    codes = np.stack([rng.integers(0, 1 << b, size=N, dtype=np.int64) for b in bits], 1).astype(np.uint16)
    return dict(bits=list(bits), cents=cents, X=X, codes=codes, eig=np.eye(L * m, dtype=np.float32))


def check(oracle, c, ks, what):
    """Every k through the best-first form against the oracle."""
    import vaq_amd
    bits, nq = c["bits"], c["X"].shape[0]
    ad = np.stack([oracle.all_dists(oracle.create_lut(c["X"][q], c["cents"], max(bits)), c["codes"]) for q in range(nq)])
    v = vaq_amd.VaqHip()
    v.mBitsAlloc = list(bits)
    v.mCentroidsPerSubs = c["cents"]
    v.mEigenVectors = c["eig"]
    v.mCodebook = c["codes"]
    for key, val in (("queries_per_pass", 1), ("early_abandon", 1), ("best_first", 1), ("timing", 1)):
        v.set_option(key, val)
    for k in ks:
        o_lab, o_dis = oracle.search(c["X"], c["cents"], c["codes"], k, max_bits=max(bits), projected=True)
        ans = v.search(c["X"], k)
        t = v.last_timing()
        assert t["best_first"] == 1, (what, k, t)
        assert_topk_matches(ans.labels.reshape(nq, k), ans.distances.reshape(nq, k), o_lab, o_dis, ad,
                            what=f"{what} k={k}")
    v.close()


def nearest_bucket_case(seed, rows_in_nearest, N=3000, nq=3, same_rows=False):
    """Bucket 0 (first code 0) is every query's nearest -- its centroid IS the queries' first L coordinates --
    and holds exactly rows_in_nearest rows."""
    c = base_case(seed, [8] * M, N, nq)
    c["cents"][0][0] = c["X"][0, :L]
    rng = np.random.default_rng(seed + 1)
    c["codes"][:, 0] = rng.integers(1, 256, size=N)
    where = rng.choice(N, rows_in_nearest, replace=False)
    c["codes"][where, 0] = 0
    if same_rows:  # the sampled rows are one row, many times: every lane minimum ties
        c["codes"][where, 1:] = c["codes"][where[0], 1:]
    return c


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 129])
def test_bootstrap_sparse_samples(vaqlib, oracle, rows):
    """The nearest bucket holds 1 .. 129 rows: fewer finite lane minima than q, exactly one wave step, fewer
    sampling waves than the workgroup has."""
    check(oracle, nearest_bucket_case(4100 + rows, rows), (100, 10), f"boot rows={rows}")


def test_bootstrap_extreme_k(vaqlib, oracle):
    """k = 1 and 100; 256 (q = 64 with four sampling waves: the last lane of the sorted wave) and 257 (q > 64:
    no bootstrap, the selection must not run)."""
    check(oracle, nearest_bucket_case(4200, 1500, N=6000), (1, 100, 256, 257), "boot k")


@pytest.mark.parametrize("rows", [40, 512])
def test_bootstrap_ties(vaqlib, oracle, rows):
    """The sampled rows are copies of one row: 32 or more of a wave's lane minima tie at the selected rank (40
    rows: the other lanes hold +inf; 512: every lane of every sampling wave ties)."""
    check(oracle, nearest_bucket_case(4300 + rows, rows, same_rows=True), (100, 17), f"boot ties rows={rows}")


@pytest.mark.parametrize("N", [100, 101, 133, BF_RANK_SORT_MAX - 1, BF_RANK_SORT_MAX, BF_RANK_SORT_MAX + 1, 3000])
def test_identical_rows_and_final_ranking(vaqlib, oracle, N):
    """Every row of the database is the same row, or one of two rows in alternation: all lane minima tie, every
    row stays admissible, and the final list -- k, k + 1, an odd count, BF_RANK_SORT_MAX - 1 / + 0 / + 1 rows, and
    a full pool -- is ordered by label within its runs of equal distance."""
    for two in (False, True):
        c = base_case(4400 + N, [8] * M, N, 2)
        c["codes"][:] = c["codes"][0]
        if two:
            c["codes"][1::2, 1:] = (c["codes"][0, 1:] + 1) % 256
        check(oracle, c, (100,), f"identical N={N} two={two}")


def flat_first_table_case(seed, buckets, N=6000, nq=2):
    """The first table is flat: the centroids of subspace 0 are the queries' first coordinates plus short vectors
    (+-8 in every coordinate, one coordinate up to +-11), so the buckets' bounds are 256 .. 313 -- many of them
    equal -- against k-th distances in the tens of thousands: no threshold excludes a bucket that has rows.
    Exactly `buckets` buckets have rows."""
    c = base_case(seed, [8] * M, N, nq)
    signs = np.array([[1.0 if (j >> b) & 1 else -1.0 for b in range(L)] for j in range(16)], np.float32)
    vecs = []
    for j in range(256):
        s = signs[j % 16].copy()
        a = j // 16
        mag = np.full(L, 8.0, np.float32)
        mag[a % L] = 8.0 + (a // L)
        vecs.append(s * mag)
    c["cents"][0] = (c["X"][0, :L][None, :] + np.array(vecs, np.float32)).astype(np.float32)
    rng = np.random.default_rng(seed + 7)
    first = rng.integers(0, buckets, size=N)
    first[:buckets] = np.arange(buckets)  # every one of them has a row
    c["codes"][:, 0] = first
    return c


@pytest.mark.parametrize("buckets", [1, 3, 4, 5, 7, 8, 9, 127, 128, 200])
def test_round_ordering(vaqlib, oracle, buckets):
    """1 .. 128 buckets in the first round (the counting loop's whole trips of eight and its tails), and 200: more
    than a round holds -- the bisection, then a second round."""
    check(oracle, flat_first_table_case(4500 + buckets, buckets), (100,), f"round buckets={buckets}")


def test_bit_packed_policy(vaqlib, oracle):
    """A C3-shaped index (bits 12, 10, 9, 8, 8, 7, 6, 4) through the bit-packed kernel: same scaffold, same code."""
    c = base_case(4600, [12, 10, 9, 8, 8, 7, 6, 4], 5003, 5)
    check(oracle, c, (100, 1), "bits")


def test_wave_primitives(vaqlib, tmp_path):
    """wave_sort64 for every rank 1..64 and wave_prefix_incl against a host sort / scan, 400 vectors
    (tests/cpp/wave_primitives_test.hip): a tiny kernel built here, run once."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "wave_primitives_test")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vaq_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "wave_primitives_test.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "wave primitives ok: 400" in r.stdout, (r.returncode, r.stdout, r.stderr)
