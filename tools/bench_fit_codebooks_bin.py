"""The binary-tree codebook fit against the flat and the hierarchical one on the README's C3 workload: 1M x 128
byte-valued rows resident in a VaqRefiner, bits {12,10,9,8,8,7,6,4}, no rotation.  Writes one JSON file (default
profiles/fit_codebooks_bin_1m.json) and prints it.

  fit        the flat fit, the hierarchical fit, the binary fit with its staged ordered sums and the binary fit with
             vaqhip_fit_codebooks_bin_set_sums(1) (the flat fit's one-thread-per-run kernel) alternate in one process,
             `--runs` repetitions each after a warm-up of all four: host clock around the call (median, min, max, every
             run); the two binary modes are asserted bit-equal on every run; the per-phase split and the tree's counts
             from vaqhip_last_fit_codebooks_bin_timing of the last run of each mode
  recall     the rows are encoded with each of the three codebooks and `--queries` queries (rows with noise added) are
             searched for k = 100: recall@100 against VaqRefiner.search's exact neighbours

No threshold is asserted.  "faster" is reported only where two ranges of run times do not overlap.

    python tools/bench_fit_codebooks_bin.py [--rows 1000000 --runs 5 --queries 1000 --out ... --commit <id>]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_fit_codebooks import D, SHAPES, make_rows, stats  # noqa: E402

K = 100


def verdict(a, sa, b, sb):
    return (f"{a} faster" if sa["max_ms"] < sb["min_ms"] else f"{b} faster" if sb["max_ms"] < sa["min_ms"] else
            "the ranges overlap: no difference reported")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_codebooks_bin_1m.json"))
    ap.add_argument("--commit", default="", help="recorded as given: the commit this build sits on")
    args = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import build, fits
    bits = SHAPES["C3"]
    M = len(bits)
    X8 = make_rows(args.rows)
    r = vaq_amd.VaqRefiner(D)
    r.set_rows_u8(X8)

    def with_sums(mode):
        def call(M_, bits_):
            fits.fit_codebooks_bin_sums(mode)
            try:
                return r.fit_codebooks_bin(M_, bits_)
            finally:
                fits.fit_codebooks_bin_sums(0)
        return call

    modes = {"flat": r.fit_codebooks, "hierarchical": r.fit_codebooks_hier, "binary_staged_sums": with_sums(0),
             "binary_one_thread_sums": with_sums(1)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(M, bits)
        return (time.perf_counter() - t0) * 1e3, res

    def same(a, b):
        return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[0], b[0]))

    first = {name: timed(fn)[1] for name, fn in modes.items()}  # warm-up of all, and the results the runs must repeat
    assert same(first["binary_staged_sums"], first["binary_one_thread_sums"])
    times = {name: [] for name in modes}
    split = {}
    for _ in range(args.runs):
        for name, fn in modes.items():
            ms, got = timed(fn)
            assert same(got, first[name]), name
            times[name].append(ms)
            if name.startswith("binary"):
                assert same(got, first["binary_staged_sums"])
                split[name] = vaq_amd.last_fit_codebooks_bin_timing()
    st = {name: stats(t) for name, t in times.items()}

    rng = np.random.default_rng(7)
    Q = X8[rng.integers(0, args.rows, args.queries)].astype(np.float32) + rng.normal(size=(args.queries, D)).astype(np.float32) * 4
    truth = r.search(Q, K).labels.reshape(-1, K)
    recall = {}
    for name in ("flat", "hierarchical", "binary_staged_sums"):
        v = vaq_amd.VaqHip()
        v.mBitsAlloc = list(bits)
        v.mCentroidsPerSubs = [np.ascontiguousarray(c) for c in first[name][0]]
        v.encode_u8(X8, projected=True)  # (no rotation: the rows are in the space the centres were fitted in)
        lab = v.search(Q, K, projected=True).labels.reshape(-1, K)
        v.close()
        recall[name.replace("_staged_sums", "")] = round(float(np.mean([len(set(a) & set(b)) / K for a, b in zip(lab, truth)])), 4)
    r.close()

    def rounded(d):
        return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in d.items()}

    out = {"workload": f"C3 {bits}: {args.rows} x {D} byte-valued rows resident in a VaqRefiner, no rotation, max_iter 25; "
                       "the four fits alternating in one process",
           "gpu": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "commit": args.commit}
    for name in modes:
        out[name] = dict(st[name], iterations=[int(i) for i in first[name][1]], nan_rows=[int(i) for i in first[name][2]])
        if name in split:
            out[name]["last_run"] = rounded(split[name])
    out.update({"binary_modes_bit_equal_on_every_run": True,
                "verdicts": {"staged sums against one-thread sums": verdict("staged sums", st["binary_staged_sums"], "one-thread sums",
                                                                            st["binary_one_thread_sums"]),
                             "binary against hierarchical": verdict("binary", st["binary_staged_sums"], "hierarchical", st["hierarchical"]),
                             "binary against flat": verdict("binary", st["binary_staged_sums"], "flat", st["flat"])},
                "recall_at_100": dict(recall, queries=args.queries, ground_truth="VaqRefiner.search (exact, all resident rows)"),
                "not_run": ["distinct GPUs (no multi-device form)", "15-bit subspaces", "1B rows"]})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
