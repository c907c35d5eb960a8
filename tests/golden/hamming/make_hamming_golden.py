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

import bitvec_cases as bc  # noqa: E402
import bitvec_ref as br  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

# name: (seed, n_bits, n, nq, k, flip): rows are a few centres with `flip` random bits turned, so distances cluster
HAMMING = {
    "hamming_w1_k10": (11, 64, 200, 4, 10, 6),
    "hamming_w3_k40_tail": (12, 150, 300, 3, 40, 10),   # 150 bits in 3 words: the 42 tail bits hold noise
    "hamming_w2_k100": (13, 128, 700, 2, 100, 8),
}
# name: (seed, W, n, k): tests/bitvec_cases.py's far crowd -- rows are the complement of query 0 with 0..3 bits turned
# back (full words), query 1 is random; the k-th best distance of query 0 is 64 W, the largest there is
FAR = {
    "hamming_w4_k260_far": (1, 4, 300, 260),
    "hamming_w16_k105_far": (1, 16, 120, 105),
}
# name: (seed, n_bits, n, nq, k, factor, D, top): raw rows are integers in [0, top)
RERANK = {
    "rerank_d16_k20_f3": (21, 128, 300, 4, 20, 3, 16, 3),
    "rerank_d7_k5_f10": (22, 64, 90, 3, 5, 10, 7, 3),
}
# name: (seed, n_bits, n, nq, k, factor, atleast, T, D): the cluster form.  Raw rows, raw queries and centres are small
# integers; factor 0: no rerank.  Every query's centre distances are distinct integers, so the visiting order is plain
# ascending order and needs no sort from anyone
CLUSTERS = {
    "clusters_w2_k20": (31, 128, 400, 3, 20, 0, 1, 6, 6),
    "clusters_w1_k30_atleast4": (32, 64, 500, 3, 30, 0, 4, 7, 6),     # atleast beyond where the walk stops by itself
    "clusters_rerank_d6_k8_f4": (33, 128, 300, 4, 8, 4, 2, 6, 6),
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
    if name in FAR:
        seed, W, n, k = FAR[name]
        n_bits, nq = 64 * W, 2
        rows, queries = bc.far_crowd(W, n=n, seed=seed)
        bc.check_far(rows, queries, k, 0)
    else:
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


def make_clusters(name):
    seed, n_bits, n, nq, k, factor, atleast, T, D = CLUSTERS[name]
    rs = np.random.RandomState(seed)
    rows, centres = bit_rows(rs, n_bits, n, 7)
    queries, _ = bit_rows(rs, n_bits, nq, 7, centres)
    top = 3
    X = rs.randint(0, top, (n, D)).astype(np.uint8)
    XQ = rs.randint(0, top, (nq, D)).astype(np.float32)
    assert D * (top - 1) ** 2 <= 32767  # float and int16 comparisons agree
    clust_idx = rs.randint(0, T, n).astype(np.int32)
    k_walk = min(factor * k, n) if factor else k
    while True:  # integer centres whose squared distances to every query are distinct
        cen = rs.randint(-2 * top, 3 * top, (T, D)).astype(np.float32)
        cd = ((XQ[:, None, :].astype(np.int64) - cen[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
        if all(len(np.unique(cd[q])) == T for q in range(nq)):
            break
    assert np.abs(np.diff(np.sort(cd, axis=1), axis=1)).min() >= 1 and cd.max() < 2 ** 24  # exact in float, well apart
    sizes = np.bincount(clust_idx, minlength=T)
    cands, n_cand = np.full((nq, n), -1, np.int32), np.zeros(nq, np.int32)
    labels = np.empty((nq, k), np.int32)
    dists = np.empty((nq, k), np.float32 if factor else np.uint32)
    ham_labels = np.empty((nq, k_walk), np.int32)
    tie = head = beyond = inside = across = False
    for q in range(nq):
        order = np.argsort(cd[q])  # (distinct: no sort's tie order is involved)
        visit = cum = 0
        for c in order:  # BitVecEngine.cpp:259-304: the centres are walked until their members number k ...
            visit += 1
            cum += sizes[c]
            if cum >= k_walk:
                break
        beyond |= visit < atleast
        visit = max(visit, atleast)  # ... and atleastCluster at least
        cand = np.concatenate([np.flatnonzero(clust_idx == c) for c in order[:visit]]).astype(np.int32)
        assert len(cand) >= k_walk
        cands[q, :len(cand)], n_cand[q] = cand, len(cand)
        h = br.hamming_dists(rows[cand], queries[q:q + 1])[0]
        idx, dh = ref_topk(h, k_walk)
        ham_labels[q] = cand[idx]
        tie |= crosses(h, k_walk)
        head |= len(np.unique(h[:k_walk])) < k_walk
        if factor:
            e = ((XQ[q][None, :].astype(np.int64) - X[ham_labels[q]].astype(np.int64)) ** 2).sum(axis=1)
            idx, de = ref_topk(e, k)
            labels[q] = ham_labels[q][idx]
            dists[q] = de.astype(np.float32)
            inside |= len(np.unique(e[:k])) < k
            across |= crosses(e, k)
        else:
            labels[q], dists[q] = ham_labels[q], dh
    assert tie, name + ": no Hamming tie across slot k"
    assert k_walk > 16 and head, name + ": no equal distances among candidates 0..k-1 with k > 16"
    assert beyond or atleast <= 2, name + ": atleast is not beyond the walk's own stopping point"
    extra = {}
    if factor:
        assert inside and across, name + ": no equal Euclidean distances inside the head and across slot k"
        extra = dict(factor=factor, X=X, hamming_labels=ham_labels)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), n_bits=n_bits, k=k, k_walk=k_walk, atleast=atleast, rows=rows,
                        queries=queries, centroids=cen, clust_idx=clust_idx, XQ=XQ, candidates=cands[:, :n_cand.max()],
                        n_cand=n_cand, labels=labels, dists=dists, **extra)
    return beyond


def main():
    assert po.have_ref(), "oracle/_ref is not built"
    assert any([make_clusters(name) for name in CLUSTERS]), "no cluster fixture with atleast beyond the walk's stop"
    big_head = [make_hamming(name) for name in list(HAMMING) + list(FAR)]
    assert any(big_head), "no Hamming fixture with k > 16 and equal distances among rows 0..k-1"
    big_head = [make_rerank(name) for name in RERANK]
    assert any(big_head), "no rerank fixture with k > 16 and equal distances inside the head"
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
