"""The exhaustive form over byte rows (vaqhip_refiner_search on a refiner filled by set_rows_u8; the uint8
instantiations of xs_tile_kernel, xs_wide_kernel and xs_replay_kernel in vaq_amd/csrc/vaq_exhaust.hip): labels and
distance bit patterns equal the float refiner's over X.astype(float32), which test_exhaustive_gpu.py pins to the
reference."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 255, 256, 257, 1000]  # the row tile (256) and either side of it
SPLITS = [0, 1, 3]
NQS = [1, 9]                   # 9: one whole block of XS_QB = 8 queries and a partial one


def equal(a, b):
    return np.array_equal(a.labels, b.labels) and np.array_equal(np.asarray(a.distances, np.float32).view(np.uint32),
                                                                 np.asarray(b.distances, np.float32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def data(D):
    """1000 byte rows with 0 and 255 in every row and some equal rows; 9 queries: continuous ones, and byte-valued ones
    (one of them a resident row) whose distances are integers, so that equal distances occur"""
    rng = np.random.default_rng(40 + D)
    X = rng.integers(0, 256, size=(1000, D), dtype=np.uint8)
    col = (np.arange(1000) * 7 + 3) % D
    X[np.arange(1000), col] = 255
    X[np.arange(1000), (col + 1) % D] = 0
    X[5::9] = X[2]
    Xq = rng.uniform(0, 255, size=(9, D)).astype(np.float32)
    Xq[0] = X[2]  # (queries 0 and 8: nq = 1 and nq = 9 both hold a byte-valued one)
    Xq[8] = rng.integers(0, 256, D)
    Xq[4] = rng.integers(0, 256, D)
    return X, Xq


@pytest.mark.parametrize("D", [7, 16, 100, 128, 129, 960])
def test_register_wide_and_replay(vaqlib, D):
    """D <= 128: the register form (7 and 100: row bases at odd addresses and at multiples of 4; 16 and 128: whole
    packets, 128 through the 16-byte loads); 129 and 960: the general path.  Every N around the tile, 1 and 3 splits
    and the automatic plan, k = 1, 10 and N + 5 (unfilled slots), one query and a partial query block; with exact_ties
    the flagged queries go through the replay."""
    import vaq_amd
    X, Xq = data(D)
    r8, rf = vaq_amd.VaqRefiner(D), vaq_amd.VaqRefiner(D)
    for N in NS:
        r8.set_rows_u8(X[:N], id_base=3)
        rf.set_rows(X[:N].astype(np.float32), id_base=3)
        for splits in SPLITS:
            r8.set_option("exhaustive_splits", splits)
            rf.set_option("exhaustive_splits", splits)
            for exact in (False, True):
                r8.exact_ties = rf.exact_ties = exact
                for k in (1, 10, N + 5):
                    for nq in NQS:
                        assert equal(r8.search(Xq[:nq], k), rf.search(Xq[:nq], k)), (D, N, splits, exact, k, nq)
    assert r8.elem_size == 1 and r8.last_search_timing()["register_form"] == (1 if D <= 128 else 0)
    r8.close(), rf.close()


@pytest.mark.parametrize("D", [16, 129])
def test_duplicate_rows_reach_the_replay(vaqlib, D):
    """1000 rows drawn from 20 distinct byte vectors: most queries hold equal distances across the k-th slot, so the
    flag step lists them and the replay over BYTE rows decides their labels -- listed_queries says that it ran"""
    import vaq_amd
    rng = np.random.default_rng(D)
    base = rng.integers(0, 256, size=(20, D), dtype=np.uint8)
    base[:, 0], base[:, 1] = 0, 255
    X = np.ascontiguousarray(base[rng.integers(0, 20, 1000)])
    Xq = rng.uniform(0, 255, size=(9, D)).astype(np.float32)
    r8, rf = vaq_amd.VaqRefiner(D), vaq_amd.VaqRefiner(D)
    r8.set_rows_u8(X)
    rf.set_rows(X.astype(np.float32))
    for r in (r8, rf):
        r.exact_ties = True
        r.set_option("timing", 1)
    for k in (1, 10, 100):
        assert equal(r8.search(Xq, k), rf.search(Xq, k)), k
        assert r8.last_search_timing()["listed_queries"] > 0, k
    r8.close(), rf.close()
