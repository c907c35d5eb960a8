"""The hierarchical codebook fit against the flat one on the README's C3 workload: 1M x 128 byte-valued rows resident
in a VaqRefiner, bits {12,10,9,8,8,7,6,4}, no rotation.  Writes one JSON file (default
profiles/fit_codebooks_hier_1m.json) and prints it.

  fit        VaqRefiner.fit_codebooks and VaqRefiner.fit_codebooks_hier alternate in one process, `--runs` repetitions
             each after a warm-up of both: host clock around the call (median, min, max, every run); the hierarchical
             fit's stage split from vaqhip_last_fit_codebooks_hier_timing of its last run
  recall     the rows are encoded with both codebooks (VaqHip.encode_u8) and `--queries` queries (rows with noise added)
             are searched for k = 100: recall@100 against VaqRefiner.search's exact neighbours, for each codebook,
             whichever way the difference comes out -- the hierarchical codebook is an approximation

No threshold is asserted.  "faster" is reported only where the two ranges of run times do not overlap.

    python tools/bench_fit_codebooks_hier.py [--rows 1000000 --runs 5 --queries 1000 --out ... --commit <id>]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_codebooks_hier_1m.json"))
    ap.add_argument("--commit", default="", help="recorded as given: the commit this build sits on")
    args = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import build
    bits = SHAPES["C3"]
    M = len(bits)
    X8 = make_rows(args.rows)
    r = vaq_amd.VaqRefiner(D)
    r.set_rows_u8(X8)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(M, bits)
        return (time.perf_counter() - t0) * 1e3, res

    _, flat = timed(r.fit_codebooks)  # warm-up of both, and the results the runs must repeat
    _, hier = timed(r.fit_codebooks_hier)
    t_flat, t_hier = [], []
    for _ in range(args.runs):
        for fn, acc, want in ((r.fit_codebooks, t_flat, flat), (r.fit_codebooks_hier, t_hier, hier)):
            ms, got = timed(fn)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[0], want[0]))
            acc.append(ms)
    split = vaq_amd.last_fit_codebooks_hier_timing()
    s_flat, s_hier = stats(t_flat), stats(t_hier)
    verdict = ("hierarchical faster" if s_hier["max_ms"] < s_flat["min_ms"] else
               "flat faster" if s_flat["max_ms"] < s_hier["min_ms"] else "the ranges overlap: no difference reported")

    rng = np.random.default_rng(7)
    Q = X8[rng.integers(0, args.rows, args.queries)].astype(np.float32) + rng.normal(size=(args.queries, D)).astype(np.float32) * 4
    truth = r.search(Q, K).labels.reshape(-1, K)
    recall = {}
    for name, cents in (("flat", flat[0]), ("hierarchical", hier[0])):
        v = vaq_amd.VaqHip()
        v.mBitsAlloc = list(bits)
        v.mCentroidsPerSubs = [np.ascontiguousarray(c) for c in cents]
        v.encode_u8(X8, projected=True)  # (no rotation: the rows are in the space the centres were fitted in)
        lab = v.search(Q, K, projected=True).labels.reshape(-1, K)
        v.close()
        recall[name] = round(float(np.mean([len(set(a) & set(b)) / K for a, b in zip(lab, truth)])), 4)
    r.close()
    out = {"workload": f"C3 {bits}: {args.rows} x {D} byte-valued rows resident in a VaqRefiner, no rotation, max_iter 25; "
                       "flat and hierarchical fit alternating in one process",
           "gpu": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "commit": args.commit,
           "flat_fit": dict(s_flat, iterations=[int(i) for i in flat[1]], nan_rows=[int(i) for i in flat[2]]),
           "hierarchical_fit": dict(s_hier, iterations=[int(i) for i in hier[1]], nan_rows=[int(i) for i in hier[2]],
                                    last_run_split={k: (round(v, 3) if isinstance(v, float) else v) for k, v in split.items()}),
           "results_bit_equal_on_every_run": True, "verdict": verdict,
           "recall_at_100": dict(recall, queries=args.queries, ground_truth="VaqRefiner.search (exact, all resident rows)"),
           "not_run": ["distinct GPUs (no multi-device form)", "15-bit subspaces (groups above 65536 rows are refused)", "1B rows"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
