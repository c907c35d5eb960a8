"""Inputs of the fixtures under tests/golden/ti_exact/ (regenerated here from a seed derived from the case's
name; the fixtures hold the outputs of the reference's loops -- VAQ::clusterTI's assignment and member sort,
the TI branch of VAQ::search, VAQ::searchTriangleInequality -- and a digest of these inputs), and the key
sequences of tests/cpp/stdsort_generic_test.cpp."""
import hashlib
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ti_exact")

N_QUERIES = 33
KS = (1, 7, 100)
VISITS = (1.0, 0.25)
METHODS = ("TI", "TI_EA")

# name -> bits per subspace, L, T, seg, rows, what the centroids / centres / queries are made of
CASES = {
    # small integer grid: equal xcc inside every cluster, equal qcc between clusters, equal distances
    "grid": dict(bits=[8] * 8, L=2, T=37, seg=2, N=4000, kind="grid"),
    "grid_bits": dict(bits=[3, 2, 2, 1], L=2, T=7, seg=2, N=3000, kind="grid"),
    # continuous: few ties (nine duplicated rows) -- the unslacked bound and bsfK * bsfK
    "cont": dict(bits=[8] * 8, L=2, T=24, seg=2, N=4000, kind="cont"),
    # two NaN centres, not at the ends: their places in the cluster order, counted by maxClusterVisit
    "nan_centres": dict(bits=[8] * 8, L=2, T=12, seg=2, N=2000, kind="nan"),
    # N in {k - 1, k, k + 1} for k = 7: the first rows_of("n_lt_k") rows of the case
    "n_lt_k": dict(bits=[3, 2, 2, 1], L=2, T=5, seg=2, N=8, kind="grid"),
}
TIE_HEAVY = ("grid", "grid_bits")
K_LARGE = 1024  # recorded on "cont" (visit 1, TI|EA) too


def rows_of(name):
    """the database sizes a case is recorded at"""
    return (6, 7, 8) if name == "n_lt_k" else (CASES[name]["N"],)


def make_inputs(name):
    """dict(bits, cents -- per subspace (1 << bits) x L float32 --, codes N x M uint16, X N_QUERIES x D float32
    (projected queries), clusters T x seg * L float32, seg)"""
    c = CASES[name]
    bits, L, T, seg, N, kind = c["bits"], c["L"], c["T"], c["seg"], c["N"], c["kind"]
    M = len(bits)
    rng = np.random.default_rng(int(hashlib.sha256(("ti_exact/" + name).encode()).hexdigest()[:8], 16))
    if kind == "grid":
        cents = [rng.integers(-2, 3, size=(1 << b, L)).astype(np.float32) for b in bits]
        X = rng.integers(-3, 4, size=(N_QUERIES, M * L)).astype(np.float32)
        clusters = rng.integers(-2, 3, size=(T, seg * L)).astype(np.float32)
        clusters[T // 2] = clusters[1]  # a copy of an earlier centre never wins the strict `<`: an empty cluster
    else:
        cents = [(rng.normal(size=(1 << b, L)) * 4).astype(np.float32) for b in bits]
        X = (rng.normal(size=(N_QUERIES, M * L)) * 4).astype(np.float32)
        clusters = (rng.normal(size=(T, seg * L)) * 4).astype(np.float32)
    codes = np.stack([rng.integers(0, 1 << b, N) for b in bits], 1).astype(np.uint16)
    if kind == "cont":
        codes[2000:2006] = codes[:6]  # nine exact duplicates
        codes[300:303] = codes[10:13]
    if kind == "nan":
        clusters[3] = np.nan
        clusters[7] = np.nan
    return dict(bits=list(bits), cents=cents, codes=codes, X=X, clusters=clusters, seg=seg)


def digest(inp):
    h = hashlib.sha256()
    arrays = [np.asarray(inp["bits"], np.int32), np.asarray([inp["seg"]], np.int32)] + list(inp["cents"]) + \
             [inp["codes"], inp["X"], inp["clusters"]]
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def key(n, k, visit, method):
    """the fixture's array names: 'lab_' / 'dis_' + key"""
    return "n%d_k%d_v%s_%s" % (n, k, ("%g" % visit).replace(".", "p"), method)


def combos(name):
    """(rows, k, visit, method) of every recorded answer of a case"""
    out = [(n, k, v, m) for n in rows_of(name) for k in KS for v in VISITS for m in METHODS]
    if name == "cont":
        out.append((CASES[name]["N"], K_LARGE, 1.0, "TI_EA"))
    return out


def load_fixture(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def sort_sequences():
    """(mode, float32 keys) for stdsort_generic_test: mode 0 = descending through an index array (clusterTI's
    member sort), 1 = ascending, NaNs allowed (the cluster order).  Lengths 0..40, 1000 and 4096; all-equal,
    few-distinct, distinct and (mode 1) NaN-bearing keys."""
    rng = np.random.default_rng(20240)
    seqs = []
    for mode in (0, 1):
        for n in list(range(0, 41)) + [1000, 4096]:
            seqs.append((mode, np.full(n, 3.0, np.float32)))
            seqs.append((mode, rng.integers(0, 4, n).astype(np.float32)))
            seqs.append((mode, rng.normal(size=n).astype(np.float32)))
            if mode == 1 and n > 0:
                for frac in (0.05, 0.3):
                    for keys in (rng.integers(0, 5, n).astype(np.float32), rng.normal(size=n).astype(np.float32)):
                        keys[rng.random(n) < frac] = np.nan
                        if n >= 3:
                            keys[n // 2] = np.nan
                        seqs.append((mode, keys))
    return seqs
