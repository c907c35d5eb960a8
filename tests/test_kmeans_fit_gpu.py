"""KMeans::fit on the GPU (vaq_kmeans_fit.hip) against tests/kmeans_fit_ref.py: centres bit for bit (NaN by position),
belongs_to and iterations equal.  The data is normal deviates (bytes for the u8 case), so the order of a sum shows in
its bits.  The assign owns 256 rows a workgroup, 32 dimensions a chunk, 64 centres a block; the update 64 dimensions a
wave, 256 member rows a tile."""
import ctypes as C

import numpy as np
import pytest

import kmeans_fit_ref as kr
from vaq_amd import VaqBitVec, VaqHipError, VaqRefiner

pytestmark = pytest.mark.gpu


def refiner(X):
    r = VaqRefiner(X.shape[1], 0)
    (r.set_rows_u8 if X.dtype == np.uint8 else r.set_rows)(X)
    return r


def normal(seed, n, D, T):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, D)).astype(np.float32), rs.choice(n, T, replace=False), 6


def u8_rows(seed, n, D, T):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (n, D)).astype(np.uint8), rs.choice(n, T, replace=False), 6


def seams():  # centre 0 holds two tiles of 256 and 88 rows, centre 1 the one far row
    X = np.random.RandomState(3).standard_normal((601, 70)).astype(np.float32)
    X[77] += 100
    return X, [0, 77], 6


def empty_cluster():  # seeds 1 and 2 are one row: centre 2 never wins, becomes NaN and keeps the fit running
    X, _, _ = normal(4, 300, 5, 3)
    return X, [10, 20, 20], 4


def equal_distances():  # row 2 is as far from centre 0 as from centre 1
    return np.array([[-1.0], [1.0], [0.0], [0.5], [-0.75]], np.float32), [0, 1], 1


def blobs():
    rs = np.random.RandomState(5)
    X = (rs.standard_normal((400, 8)) + 50 * (np.arange(400) % 4)[:, None]).astype(np.float32)
    return X, [0, 1, 2, 3], 25


CASES = {"n255_D1_T1": lambda: normal(1, 255, 1, 1), "n257_D31_T63": lambda: normal(2, 257, 31, 63),
         "n1025_D33_T65": lambda: normal(6, 1025, 33, 65), "n257_D130_T65": lambda: normal(7, 257, 130, 65),
         "u8_D33_T65": lambda: u8_rows(8, 300, 33, 65), "seams": seams, "empty_cluster": empty_cluster,
         "equal_distances": equal_distances, "root": lambda: kr.root_case() + (1,), "blobs": blobs}


@pytest.mark.parametrize("case", list(CASES))
def test_fit(vaqlib, case):
    import torch
    X, seeds, max_iter = CASES[case]()
    want = kr.fit(X, seeds, max_iter)
    r = refiner(X)
    got = r.fit_centres(len(seeds), seeds, max_iter)
    if case in ("n1025_D33_T65", "u8_D33_T65"):  # the _device form, on a stream of its own
        with torch.cuda.stream(torch.cuda.Stream()):
            dev = r.fit_centres_device(len(seeds), torch.tensor(seeds, dtype=torch.int32).cuda(), max_iter)
        assert dev[2] == got[2] and np.array_equal(dev[0].cpu().numpy(), got[0], equal_nan=True) and np.array_equal(dev[1].cpu().numpy(), got[1])
    print(case, "iterations", got[2], "members", np.bincount(got[1], minlength=len(seeds))[:4])
    assert got[2] == want[2] and np.array_equal(got[1], want[1])
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    assert np.array_equal(got[0].view(np.uint32)[~np.isnan(want[0])], want[0].view(np.uint32)[~np.isnan(want[0])])
    members = np.bincount(got[1], minlength=len(seeds))
    if case == "seams":
        assert members[0] >= 2 * 256 + 1 and members[1] == 1
    if case == "empty_cluster":
        assert members[2] == 0 and np.isnan(got[0][2]).all() and got[2] == max_iter
    if case in ("equal_distances", "root"):
        assert got[1][2] == 0
    if case == "blobs":  # converged: the assignment is the centres' own cluster index
        assert got[2] < max_iter
        rs = np.random.RandomState(9)
        bits, XQ = rs.randint(0, 2 ** 62, (400, 1)).astype(np.uint64), X[rs.choice(400, 6)] + np.float32(0.25)
        answers = []
        for from_refiner in (True, False):
            bv = VaqBitVec(0, 64)
            bv.set_rows(bits)
            bv.set_clusters_from_refiner(got[0], r) if from_refiner else bv.set_clusters(got[0], got[1])
            answers.append(bv.query_naive_clusters(XQ, 9, r, atleast_cluster=2))
            bv.close()
        assert all(np.array_equal(a, b) for a, b in zip(*answers))
    r.close()


@pytest.mark.parametrize("case,code,text", [("seed_negative", -1, "seed_rows[1]"), ("seed_n", -1, "seed_rows[2]"),
                                            ("seed_n_device", -1, "seed_rows[2]"), ("empty_refiner", -7, "no rows"),
                                            ("nan_row", -1, "row 3 ")])
def test_refusals(vaqlib, case, code, text):
    import torch
    X, seeds, _ = normal(11, 300, 5, 3)
    seeds = {"seed_negative": [4, -1, 5], "seed_n": [4, 5, 300], "seed_n_device": [4, 5, 300]}.get(case, list(seeds))
    if case == "nan_row":
        X[3, 2] = np.nan
    r = VaqRefiner(5, 0) if case == "empty_refiner" else refiner(X)
    if case == "seed_n_device":
        with pytest.raises(VaqHipError) as e:
            r.fit_centres_device(3, torch.tensor(seeds, dtype=torch.int32).cuda())
        assert e.value.code == code and text in str(e.value)
    else:  # the C entry itself: no refusal writes an output
        s, cen, idx, it = np.array(seeds, np.int32), np.full((3, 5), 77, np.float32), np.full(300, 77, np.int32), C.c_int(77)
        rc = vaqlib.vaqhip_refiner_fit_centres(r._h, 3, s.ctypes.data, 25, cen.ctypes.data, idx.ctypes.data, C.byref(it))
        assert rc == code and text in vaqlib.vaqhip_last_error().decode()
        assert (cen == 77).all() and (idx == 77).all() and it.value == 77
    r.close()
