"""Records tests/golden/hamming/*.npz on the CPU from the compiled reference's KNNFromDists<int16_t>
(oracle.pyoracle.ref_knn_from_dists; oracle/_ref must be built).  Run from the repository root:

    python tests/golden/hamming/make_hamming_golden.py

Every fixture is checked against the conditions that make it worth having (README.md) before it is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bitvec_ref as br  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

# name: (seed, n_bits, n, nq, k, flip): rows are a few centres with `flip` random bits turned, so distances cluster
HAMMING = {
    "hamming_w1_k10": (11, 64, 200, 4, 10, 6),
    "hamming_w3_k40_tail": (12, 150, 300, 3, 40, 10),   # 150 bits in 3 words: the 42 tail bits hold noise
    "hamming_w2_k100": (13, 128, 700, 2, 100, 8),
}
# name: (seed, n_bits, n, nq, k, factor, D, top): raw rows are integers in [0, top)
RERANK = {
    "rerank_d16_k20_f3": (21, 128, 300, 4, 20, 3, 16, 3),
    "rerank_d7_k5_f10": (22, 64, 90, 3, 5, 10, 7, 3),
}


def bit_rows(rs, n_bits, n, flip, centres=None):
    W = (n_bits + 63) // 64
    if centres is None:
        centres = rs.randint(0, 256, (5, W * 8)).astype(np.uint8)
    rows = centres[rs.randint(0, centres.shape[0], n)].copy()
    for r in range(n):
        for b in rs.randint(0, W * 64, flip):  # any bit of any word, the tail included
            rows[r, b // 8] ^= np.uint8(1 << (b % 8))
    return np.ascontiguousarray(rows).view(np.uint64).reshape(n, W), centres


def ref_topk(d, k):
    """the compiled reference on the int16 cast of one query's distances"""
    assert d.max() <= 32767
    idx, dist = po.ref_knn_from_dists(d.astype(np.int16), k)
    return idx.astype(np.int32), dist.astype(np.int64)


def crosses(d, k):
    s = np.sort(d)
    return len(s) > k and s[k - 1] == s[k]


def make_hamming(name):
    seed, n_bits, n, nq, k, flip = HAMMING[name]
    rs = np.random.RandomState(seed)
    rows, centres = bit_rows(rs, n_bits, n, flip)
    queries, _ = bit_rows(rs, n_bits, nq, flip, centres)
    d = br.hamming_dists(rows, queries)
    labels = np.empty((nq, k), np.int32)
    dists = np.empty((nq, k), np.uint32)
    for q in range(nq):
        labels[q], dq = ref_topk(d[q], k)
        dists[q] = dq
    assert any(crosses(d[q], k) for q in range(nq)), name + ": no run of equal distances crosses slot k"
    head_ties = any(len(np.unique(d[q, :k])) < k for q in range(nq))
    if n_bits % 64:
        tail = rows[:, -1] & np.uint64((1 << (64 - n_bits % 64)) - 1)  # dimension d is bit 63 - d % 64: the tail is low
        assert tail.any(), name + ": the tail bits hold nothing"
    np.savez_compressed(os.path.join(HERE, name + ".npz"), n_bits=n_bits, k=k, rows=rows, queries=queries, labels=labels,
                        dists=dists)
    return k > 16 and head_ties


def make_rerank(name):
    seed, n_bits, n, nq, k, factor, D, top = RERANK[name]
    rs = np.random.RandomState(seed)
    rows, centres = bit_rows(rs, n_bits, n, 7)
    queries, _ = bit_rows(rs, n_bits, nq, 7, centres)
    X = rs.randint(0, top, (n, D)).astype(np.uint8)
    XQ = rs.randint(0, top, (nq, D)).astype(np.float32)
    assert D * (top - 1) ** 2 <= 32767  # float and int16 comparisons agree
    k_temp = min(factor * k, n)
    d = br.hamming_dists(rows, queries)
    labels = np.empty((nq, k), np.int32)
    dists = np.empty((nq, k), np.float32)
    cand_all = np.empty((nq, k_temp), np.int32)
    inside = across = False
    for q in range(nq):
        cand, _ = ref_topk(d[q], k_temp)
        cand_all[q] = cand
        e = ((XQ[q][None, :].astype(np.int64) - X[cand].astype(np.int64)) ** 2).sum(axis=1)
        idx, de = ref_topk(e, k)
        labels[q] = cand[idx]
        dists[q] = de.astype(np.float32)
        inside |= len(np.unique(e[:k])) < k
        across |= crosses(e, k)
    assert inside, name + ": no equal Euclidean distances inside the head"
    assert across, name + ": no equal Euclidean distances across slot k"
    assert any(crosses(d[q], k_temp) for q in range(nq)), name + ": no Hamming tie across slot kTemp"
    np.savez_compressed(os.path.join(HERE, name + ".npz"), n_bits=n_bits, k=k, factor=factor, rows=rows, queries=queries,
                        X=X, XQ=XQ, candidates=cand_all, labels=labels, dists=dists)
    return k > 16 and inside


def main():
    assert po.have_ref(), "oracle/_ref is not built"
    big_head = [make_hamming(name) for name in HAMMING]
    assert any(big_head), "no Hamming fixture with k > 16 and equal distances among rows 0..k-1"
    big_head = [make_rerank(name) for name in RERANK]
    assert any(big_head), "no rerank fixture with k > 16 and equal distances inside the head"
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
