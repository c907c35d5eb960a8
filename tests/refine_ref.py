"""NumPy restatement of VAQ::refine (VAQ.cpp:849-876) with the reference's own numbers, and the inputs of the
fixtures under tests/golden/refine/ (regenerated here from a seed; the fixtures hold the reference's outputs and a
digest of these inputs).

  * the distance is (XTest.row(q) - XTrain.row(l)).squaredNorm(): Eigen's linear vectorised reduction, restated for
    the k-means already (kmeans_ref.sqnorm_eigen) -- not the sequential dist += t * t;
  * the k best are what the reference's heap leaves (utils/Heap.hpp, CMax<float, int>): heap_heapify to FLT_MAX / -1,
    then per candidate, in candidate order, heap_pop + heap_push when heap_top > dist, then heap_reorder.  RefHeap
    below restates it statement for statement, as vaq::refheap (vaq_amd/csrc/vaq_restated.h) does for the kernels.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

import kmeans_ref as kr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine")
FLT_MAX = np.finfo(np.float32).max

# name: kind ("cont": near-duplicate continuous rows, "int": integer rows from few distinct vectors), D, N, nq, R,
# ks, distinct vectors the rows are built from, dup (candidates drawn WITH repetition from this many rows, 0 = distinct),
# draw (which draw of the case's seed; default 0)
CASES = {
    # the paths of Eigen's reduction: no packet, one packet, one packet + tail, two packets, the loop + odd packet,
    # loop + odd packet (none) + tail, the loop alone, loop + tail of one, a long loop
    "cont_d7": dict(kind="cont", D=7, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d8": dict(kind="cont", D=8, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d12": dict(kind="cont", D=12, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d16": dict(kind="cont", D=16, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d40": dict(kind="cont", D=40, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d100": dict(kind="cont", D=100, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d128": dict(kind="cont", D=128, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d129": dict(kind="cont", D=129, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    "cont_d960": dict(kind="cont", D=960, N=300, nq=4, R=200, ks=(10, 100), distinct=20, dup=0),
    # integer rows: every sum is exact, the heap alone decides the labels.  The draw is the first on which EVERY query
    # has a tie across the k-th slot for k = 1, 10 and 100 (test_refine_exact_cpu.py keeps that true)
    "int_ties": dict(kind="int", D=32, N=300, nq=6, R=200, ks=(1, 10, 100, 200), distinct=20, dup=0, draw=4),
    "dup_cands": dict(kind="cont", D=24, N=300, nq=4, R=64, ks=(1, 16, 64), distinct=20, dup=40),
    "r1": dict(kind="cont", D=128, N=300, nq=4, R=1, ks=(1,), distinct=20, dup=0),
    "r2048": dict(kind="int", D=16, N=3000, nq=2, R=2048, ks=(1, 100, 2048), distinct=40, dup=0),
}
CONTINUOUS = [n for n, c in CASES.items() if n.startswith("cont_")]
NOISE = 2e-4  # half width of what a "cont" row adds to its base vector: candidates a few ulps apart in distance


def make_inputs(name: str):
    """(XTest nq x D, XTrain N x D, cand nq x R int32) of a case, from its fixed seed."""
    c = CASES[name]
    rng = np.random.default_rng(int(hashlib.sha256(("refine/%s/%d" % (name, c.get("draw", 0))).encode()).hexdigest()[:8], 16))
    D, N, nq, R = c["D"], c["N"], c["nq"], c["R"]
    if c["kind"] == "int":
        base = rng.integers(0, 256, size=(c["distinct"], D)).astype(np.float32)
        Xt = base[rng.integers(0, c["distinct"], N)]
        Xq = rng.integers(0, 256, size=(nq, D)).astype(np.float32)
    else:
        base = rng.uniform(0, 255, size=(c["distinct"], D)).astype(np.float32)
        Xt = (base[rng.integers(0, c["distinct"], N)] + rng.uniform(-NOISE, NOISE, size=(N, D)).astype(np.float32))
        Xt = Xt.astype(np.float32)
        Xq = rng.uniform(0, 255, size=(nq, D)).astype(np.float32)
    if c["dup"]:
        cand = rng.integers(0, c["dup"], size=(nq, R))
    else:
        cand = np.stack([rng.permutation(N)[:R] for _ in range(nq)])
    return np.ascontiguousarray(Xq), np.ascontiguousarray(Xt), np.ascontiguousarray(cand.astype(np.int32))


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def load_fixture(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


class RefHeap:
    """utils/Heap.hpp, CMax<float, int> over k slots (1-based inside, as the reference indexes it)."""

    def __init__(self, k: int):
        self.k = k
        self.val = [FLT_MAX] * (k + 1)  # heap_heapify of nothing (:211-235); slot 0 unused
        self.ids = [-1] * (k + 1)

    def top(self):
        return self.val[1]

    def pop(self, k=None):  # :115-144
        k = self.k if k is None else k
        val, ids = self.val, self.ids
        v = val[k]
        i = 1
        while True:
            i1 = i << 1
            i2 = i1 + 1
            if i1 > k:
                break
            if i2 == k + 1 or val[i1] > val[i2]:
                if v > val[i1]:
                    break
                val[i], ids[i] = val[i1], ids[i1]
                i = i1
            else:
                if v > val[i2]:
                    break
                val[i], ids[i] = val[i2], ids[i2]
                i = i2
        val[i], ids[i] = val[k], ids[k]

    def push(self, v, idx):  # :151-169
        val, ids = self.val, self.ids
        i = self.k
        while i > 1:
            f = i >> 1
            if not (v > val[f]):
                break
            val[i], ids[i] = val[f], ids[f]
            i = f
        val[i], ids[i] = v, idx

    def reorder(self):  # :322-349 -> (labels, distances), ascending, unfilled slots -1 / FLT_MAX
        k = self.k
        ii = 0
        for i in range(k):
            v, idx = self.val[1], self.ids[1]
            self.pop(k - i)
            self.val[k - ii], self.ids[k - ii] = v, idx
            if idx != -1:
                ii += 1
        lab = self.ids[k - ii + 1:k + 1] + [-1] * (k - ii)
        dis = self.val[k - ii + 1:k + 1] + [FLT_MAX] * (k - ii)
        return np.array(lab, np.int32), np.array(dis, np.float32)


def distances(Xq, Xt, cand, order="eigen", id_base=0):
    """float32 nq x R; candidates outside [id_base, id_base + N) (the skipped ones) get +inf."""
    Xq = np.asarray(Xq, np.float32)
    Xt = np.asarray(Xt, np.float32)
    row = np.asarray(cand, np.int64) - id_base
    ok = (np.asarray(cand) >= 0) & (row >= 0) & (row < len(Xt))
    diff = Xq[:, None, :] - Xt[np.where(ok, row, 0)]
    red = kr.sqnorm_eigen if order == "eigen" else kr.sqnorm_sequential
    with np.errstate(invalid="ignore", over="ignore"):
        d = red(diff * diff)
    assert d.dtype == np.float32
    return np.where(ok, d, np.float32(np.inf))


def heap_topk(dist_row, cand_row, k):
    """VAQ.cpp:863-872 for one query over its R distances in candidate order."""
    h = RefHeap(k)
    for d, l in zip(dist_row.tolist(), cand_row.tolist()):
        if h.top() > d:
            h.pop()
            h.push(d, l)
    return h.reorder()


def smallest_label_topk(dist_row, cand_row, k):
    """The k smallest admissible candidates by (distance, label); duplicates kept."""
    keep = np.nonzero(dist_row < FLT_MAX)[0]
    o = keep[np.lexsort((cand_row[keep], dist_row[keep]))][:k]
    lab = np.full(k, -1, np.int32)
    dis = np.full(k, FLT_MAX, np.float32)
    lab[:len(o)] = cand_row[o]
    dis[:len(o)] = dist_row[o]
    return lab, dis


def refine(Xq, Xt, cand, k, exact=True, order="eigen", id_base=0):
    """(labels nq x k int32, distances nq x k float32)."""
    cand = np.asarray(cand, np.int32)
    d = distances(Xq, Xt, cand, order, id_base)
    pick = heap_topk if exact else smallest_label_topk
    out = [pick(d[q], cand[q], k) for q in range(len(cand))]
    if not out:
        return np.empty((0, k), np.int32), np.empty((0, k), np.float32)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def boundary_ties(dist_row, k) -> bool:
    """Is the k-th smallest distance of the candidates equal to the (k+1)-th?"""
    s = np.sort(dist_row)
    return k < len(s) and s[k - 1] == s[k]


def assert_default_rule(labels, dists, want_labels, want_dists, what=""):
    """What a refine without "exact_ties" owes the reference's answer: the distances slot for slot, and the labels
    after sorting each run of equal distances by label -- except in the LAST run when it is cut by k (the same
    distance continues past the k-th slot): there the heap and the (distance, label) rule may keep different
    members, and only the comparison with the restated rule itself (made by the caller) says which."""
    labels, dists = np.asarray(labels), np.asarray(dists, np.float32)
    assert np.array_equal(dists.view(np.uint32), np.asarray(want_dists, np.float32).view(np.uint32)), what
    nq, k = labels.shape
    for q in range(nq):
        s = 0
        for i in range(1, k + 1):
            if i == k or dists[q, i] != dists[q, s]:
                a, b = labels[q, s:i], np.asarray(want_labels)[q, s:i]
                if not np.array_equal(np.sort(a), np.sort(b)):
                    assert i == k, f"{what}: q{q} run {s}:{i} holds other labels"
                s = i
