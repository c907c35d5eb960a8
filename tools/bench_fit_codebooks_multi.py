"""The sharded codebook fit (vaqhip_multi_refiner_fit_codebooks) against the single fit over resident rows
(vaqhip_refiner_fit_codebooks) at 1M x 128 byte-valued rows, the workload of tools/bench_fit_codebooks.py: shapes C2
(8 x 8 bits), C3 (12,10,9,8,8,7,6,4) and FAST (64 x 4 bits), the rows resident as bytes in a refiner.
Writes one JSON file (default profiles/fit_codebooks_multi_1m.json) and prints it.  Per shape the single fit and the
sharded fit at G = 1, 2, 4, 8 alternate in one process, --runs repetitions after a warm-up of each; medians with
min-max, the per-phase split of the last sharded run (slowest device, device events; total_ms is the library's own
wall time of the call, teardown included), one more run of every form with the fit's phase times, and every result,
those runs' included, asserted bit-equal to the single fit's.
The shards are LOGICAL shards of one GPU: the figures are the cost of the mechanism (shard step, exchange, G owner
pipelines sharing one device), not scaling.  Distinct GPUs and anything near 1B rows: NOT MEASURED.

    python tools/bench_fit_codebooks_multi.py [--rows 1000000 --runs 5 --out FILE --commit <id>]
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

GS = (1, 2, 4, 8)


def bits_of(fit):
    cents, iters, nan = fit
    return [c.view(np.uint32) for c in cents], iters, nan


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def overlap(a, b):
    return not (a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_codebooks_multi_1m.json"))
    ap.add_argument("--commit", default="", help="recorded as given: the commit this build sits on")
    args = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import build
    X8 = make_rows(args.rows)
    one = vaq_amd.VaqRefiner(D, device=args.device)
    one.set_rows_u8(X8)
    many = {}
    for G in GS:
        many[G] = vaq_amd.VaqMultiRefiner([args.device] * G, D)
        many[G].set_rows_u8(X8)

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return (time.perf_counter() - t0) * 1e3, bits_of(r)

    out = {"workload": f"KMeans::staticFitSampling per subspace, max_iter 25: {args.rows} x {D} byte-valued rows resident as "
                       "bytes in a refiner, no rotation; the single fit and the sharded fit at G = 1, 2, 4, 8 alternating",
           "shards": "LOGICAL shards of ONE GPU: the cost of the mechanism, not scaling",
           "distinct_gpus": "NOT MEASURED", "near_1b_rows": "NOT MEASURED",
           "gpu": torch.cuda.get_device_name(args.device), "source_hash": build.source_hash(), "commit": args.commit, "shapes": {}}
    for name, bits in SHAPES.items():
        M = len(bits)
        _, want = timed(lambda: one.fit_codebooks(M, bits))  # warm-up of every form, and the yardstick
        for G in GS:
            assert same(timed(lambda: many[G].fit_codebooks(M, bits))[1], want), (name, G)
        t_one, t_many, phases = [], {G: [] for G in GS}, {}
        for _ in range(args.runs):
            ms, got = timed(lambda: one.fit_codebooks(M, bits))
            assert same(got, want), name
            t_one.append(ms)
            for G in GS:
                ms, got = timed(lambda: many[G].fit_codebooks(M, bits))
                assert same(got, want), (name, G)
                t_many[G].append(ms)
                t = vaq_amd.last_multi_fit_codebooks_timing()
                phases[G] = {k: round(t[k], 3) for k in ("total_ms", "columns_ms", "copy_ms", "place_ms")}
                phases[G]["owner_subspaces"] = t["owner_subspaces"]
        # one more run of every form with phase times (a synchronisation per phase): the single fit's, the owners'
        vaq_amd.fit_codebooks_timing(True)
        assert same(bits_of(one.fit_codebooks(M, bits)), want), name
        t = vaq_amd.last_fit_codebooks_timing()
        single_phases = {k: round(t[k], 3) for k in ("gather_ms", "assign_ms", "accumulate_ms", "update_ms")}
        for G in GS[1:]:
            assert same(bits_of(many[G].fit_codebooks(M, bits)), want), (name, G)
            t = vaq_amd.last_multi_fit_codebooks_timing()
            phases[G]["owner_phases_with_synchronisations_ms"] = {k: round(t[k], 3) for k in ("assign_ms", "accumulate_ms", "update_ms")}
        vaq_amd.fit_codebooks_timing(False)
        s_one = stats(t_one)
        s_one["phases_with_synchronisations_ms"] = single_phases
        res = {"bits": bits, "iterations": want[1].tolist(), "results_bit_equal_on_every_run": True,
               "vaqhip_refiner_fit_codebooks": s_one, "vaqhip_multi_refiner_fit_codebooks": {}}
        for G in GS:
            s = stats(t_many[G])
            s["last_phases_ms"] = phases[G]
            s["ranges_overlap_with_single"] = overlap(s, s_one)
            s["faster_than_single"] = s["max_ms"] < s_one["min_ms"]
            res["vaqhip_multi_refiner_fit_codebooks"][str(G)] = s
        out["shapes"][name] = res
        print(name, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
