"""Key sequences for the std::sort restatements (vaq::stdsort::sort in vaq_fast.h and
fast_ref.std_sort_perm): the shapes a quicksort is sensitive to, and adversarial ones that
drive the introsort past its depth limit into the heap-sort fallback.

The adversary is McIlroy's ("A Killer Adversary for Quicksort", 1999) played against the
Python restatement: every key starts as "gas" (larger than any fixed key, value undecided);
when two gas items are compared one of them is frozen to the next fixed value, and every
comparison is answered from the values so far.  The answers are consistent with the final
keys, so the sort takes the same path when it is run again on them with the ordinary
comparator -- which heap_sort_calls() lets a test assert rather than believe.
Every key is <= n <= 1024: it fits the 16-bit key of the device form."""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np

import fast_ref as fr

ADVERSARIAL_N = (64, 100, 257, 1000, 1023, 1024, 65, 128, 500, 777)


def adversarial_keys(n: int) -> np.ndarray:
    """n keys in [0, n] on which the restated introsort degenerates."""
    gas = n
    val = [gas] * n
    state = {"solid": 0, "cand": 0}

    def lt(a, b):
        x, y = a[0], b[0]
        if val[x] == gas and val[y] == gas:
            z = x if x == state["cand"] else y
            val[z] = state["solid"]
            state["solid"] += 1
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]

    saved = fr._lt
    fr._lt = lt
    try:
        fr.std_sort_perm(np.zeros(n, np.int64))
    finally:
        fr._lt = saved
    return np.array(val, np.int64)


def adversarial_tied(n: int, group: int) -> np.ndarray:
    """adversarial_keys(n) with ties where the permutation of equal keys is decided by the heap sort:
    the items of the heap-sorted sub-range keep their order but share a key `group` at a time (all one
    key when group >= the sub-range's length).  Items left of the sub-range stay <=, items right >=."""
    keys = adversarial_keys(n)
    ranges = []
    saved = fr._heap_sort

    def capture(f, lo, hi):
        ranges.append([p[0] for p in f[lo:hi]])
        return saved(f, lo, hi)

    fr._heap_sort = capture
    try:
        fr.std_sort_perm(keys)
    finally:
        fr._heap_sort = saved
    if not ranges:
        return keys
    rows = np.array(ranges[0])
    rows = rows[np.argsort(keys[rows], kind="stable")]
    keys[rows] = keys[rows].min() + np.arange(len(rows)) // group
    return keys


def adversarial_sequences():
    """[(name, n, keys)]: distinct keys, then pairs, fives and one run of equal keys in the fallback's range"""
    out = []
    for n in ADVERSARIAL_N:
        out.append((f"adversarial_{n}", n, adversarial_keys(n)))
        for g in (2, 5, n):
            out.append((f"adversarial_{n}_tied{g}", n, adversarial_tied(n, g)))
    return out


@contextmanager
def heap_sort_calls():
    """Counts fast_ref._heap_sort calls: yields a list that receives each call's sub-range length."""
    calls = []
    saved = fr._heap_sort

    def counted(f, lo, hi):
        calls.append(hi - lo)
        return saved(f, lo, hi)

    fr._heap_sort = counted
    try:
        yield calls
    finally:
        fr._heap_sort = saved


def reaches_heap_sort(keys) -> list:
    """sub-range lengths heap-sorted when the checker sorts `keys` with the ordinary comparator"""
    with heap_sort_calls() as calls:
        fr.std_sort_perm(keys)
    return list(calls)


def shaped_sequences(seed: int = 2024):
    """[(name, keys)]: every n in 1..1024 at least once, the sizes around the insertion-sort
    threshold, few / some / all-distinct random keys, and the classic quicksort shapes."""
    rng = np.random.default_rng(seed)
    out = []
    kinds = ("one", "two", "three", "sqrt", "full", "asc", "desc", "organ", "saw")

    def make(kind, n):
        i = np.arange(n, dtype=np.int64)
        if kind == "one":
            return np.full(n, int(rng.integers(0, 1025)), np.int64)
        if kind == "two":
            return rng.integers(0, 2, n).astype(np.int64) * 7 + 3
        if kind == "three":
            return rng.integers(0, 3, n).astype(np.int64)
        if kind == "sqrt":
            return rng.integers(0, max(2, int(np.sqrt(n))), n).astype(np.int64)
        if kind == "full":
            return rng.integers(0, max(2, min(n, 1025)), n).astype(np.int64)
        if kind == "asc":
            return i.copy()
        if kind == "desc":
            return (n - 1 - i)
        if kind == "organ":
            return np.minimum(i, n - 1 - i)
        return i % max(2, n // 7 + 1)  # sawtooth

    for n in range(1, 1025):  # every n once, the kind cycling
        kind = kinds[n % len(kinds)]
        out.append((f"{kind}_{n}", make(kind, n)))
    for n in (15, 16, 17, 32, 33, 64, 100, 255, 256, 257, 1000, 1023, 1024):  # every kind at the edges
        for kind in kinds:
            out.append((f"{kind}_{n}", make(kind, n)))
    for t in range(40):
        n = int(rng.integers(18, 1025))
        out.append((f"sqrt_{n}_r{t}", make("sqrt", n)))
    return out
