#!/usr/bin/env python
"""Time the exhaustive form of the resident refiner (vaqhip_refiner_search_device) against the only route a user had
before it: vaqhip_refiner_refine_device over slabs of 2048 consecutive labels plus vaqhip_merge_topk_device.

  python tools/bench_exhaustive.py [--rows 1000000] [--dim 128] [--queries 100,10000] [--k 100] [--reps 5]
                                   [--warmup 2] [--exact-queries 100] [--out profiles/exhaustive_1m.json]

Two data sets: harness.sift_like (integer-valued, SIFT-shaped) and a tie-heavy one (rows copied from 1000 distinct
integer vectors: every query has equal distances among its best).  Per data set and number of queries the two routes
are alternated inside one process, each repetition timed with device events around the enqueued calls (median, min,
max).  Before anything is timed the two answers are compared, labels and distance bits.  Beside the times:
  lane_ops            3 * nq * N * D (sub, mul, add per element and pair)
  vector_rate_share   lane_ops / select time / 39.3e12 (1024 SIMDs x 16 lanes x 2.4 GHz)
  phases              one extra, untimed-by-events call with option "timing" (it synchronises between phases)
With --exact-queries n > 0 the same is done with "exact_ties" for the first n queries: the replay's wall time and the
rate at which the listed queries together stream the rows (listed * N * D * 4 bytes / replay time).
The slab route's timing holds what its user pays: 489 label updates and launches per call plus the merge levels (their
buffers are made once, outside the timing); at 100 queries that is bound by the launches, not by the device.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLAB = 2048
VECTOR_RATE = 39.3e12


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", default="100,10000")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exact-queries", type=int, default=100)
    ap.add_argument("--exact-only", type=int, default=0, help="1: only the exact_ties leg")
    ap.add_argument("--data", default="sift_like,tie_heavy")
    ap.add_argument("--skip-slabs", type=int, default=0, help="1: time the new call alone (profiling runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    import vaq_amd
    from vaq_amd import _lib, build, harness
    from vaq_amd.index import merge_topk_device
    if not torch.cuda.is_available():
        print("bench_exhaustive: no GPU: nothing is measured", file=sys.stderr)
        return 1
    L = _lib.load()
    N, D, k = a.rows, a.dim, a.k
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    nqs = [int(x) for x in a.queries.split(",")]
    n_slabs = (N + SLAB - 1) // SLAB
    out = {"rows": N, "dim": D, "k": k, "reps": a.reps, "warmup": a.warmup, "slab": SLAB,
           "device": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "cases": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for data in a.data.split(","):
        if data == "sift_like":
            rows = harness.sift_like(N, D, stream=0, device=dev)
            queries = harness.sift_like(max(nqs), D, stream=1, device=dev)
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(17)
            base = torch.randint(0, 256, (1000, D), generator=g, device=dev).float()
            rows = base[torch.randint(0, 1000, (N,), generator=g, device=dev)].contiguous()
            queries = torch.randint(0, 256, (max(nqs), D), generator=g, device=dev).float()
        r = vaq_amd.VaqRefiner(D)
        r.set_rows(rows)
        legs = [] if a.exact_only else [(n, 0) for n in nqs]
        for nq, exact in legs + ([(min(a.exact_queries, max(nqs)), 1)] if a.exact_queries > 0 else []):
            q = queries[:nq].contiguous()
            r.exact_ties = bool(exact)
            ol = torch.empty((nq, k), dtype=torch.int32, device=dev)
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)

            def new():
                _lib.check(L.vaqhip_refiner_search_device(r._h, p(q), nq, k, p(ol), p(od), C.c_void_p(st)))

            calls = {"search_device": new}
            if not a.skip_slabs:
                lab0 = torch.arange(SLAB, dtype=torch.int32, device=dev).repeat(nq, 1).contiguous()
                lab = torch.empty_like(lab0)
                pl = torch.empty((n_slabs, nq, k), dtype=torch.int32, device=dev)
                pd = torch.empty((n_slabs, nq, k), dtype=torch.float32, device=dev)
                sl, sd = torch.empty_like(ol), torch.empty_like(od)

                # the merge's levels (vaqhip_merge_topk_device takes 16 lists): buffers made once, outside the timing
                levels, n = [], n_slabs
                while n > 16:
                    n = (n + 15) // 16
                    levels.append((torch.empty((n, nq, k), dtype=torch.int32, device=dev),
                                   torch.empty((n, nq, k), dtype=torch.float32, device=dev)))

                def slabs():  # (labels at or past N are skipped by the kernel: the last slab may be short)
                    for s in range(n_slabs):
                        torch.add(lab0, s * SLAB, out=lab)
                        _lib.check(L.vaqhip_refiner_refine_device(r._h, p(q), nq, p(lab), SLAB, k, p(pl[s]), p(pd[s]),
                                                                  C.c_void_p(st)))
                    cl, cd = pl, pd
                    for nl, nd in levels:
                        for g in range(nl.shape[0]):
                            merge_topk_device(cd[16 * g:16 * g + 16], cl[16 * g:16 * g + 16], k, out=(nl[g], nd[g]))
                        cl, cd = nl, nd
                    merge_topk_device(cd, cl, k, out=(sl, sd))

                calls["slab_route"] = slabs
                new()
                slabs()
                torch.cuda.synchronize()
                same = bool(torch.equal(ol, sl) and torch.equal(od.view(torch.int32), sd.view(torch.int32)))
                if not exact:  # (with exact_ties the slab route merges by (distance, label): not the heap's order)
                    assert same, "search_device != slabs + merge"
            times = {n: [] for n in calls}
            for it in range(a.warmup + a.reps):
                for n, fn in calls.items():  # alternated: one of each per repetition
                    ms = timed(fn)
                    if it >= a.warmup:
                        times[n].append(ms)
            r.set_option("timing", 1)
            new()
            ph = r.last_search_timing()
            r.set_option("timing", 0)
            lane_ops = 3 * nq * N * D
            case = {"data": data, "queries": nq, "exact_ties": exact, "lane_ops": lane_ops,
                    "phases": {n: (round(v, 4) if isinstance(v, float) else v) for n, v in ph.items()}}
            for n in calls:
                case[n + "_ms"] = stats(times[n])
            case["vector_rate_share_of_select"] = round(lane_ops / (ph["select_ms"] * 1e-3) / VECTOR_RATE, 4)
            case["vector_rate_share_of_call"] = round(lane_ops / (case["search_device_ms"]["median"] * 1e-3) / VECTOR_RATE, 4)
            if not a.skip_slabs:
                case["matches_slab_route"] = same
                case["speedup_vs_slab_route"] = round(case["slab_route_ms"]["median"] / case["search_device_ms"]["median"], 3)
            if exact and ph["listed_queries"]:
                # one workgroup per listed query, side by side: replay_ms is the wall time of ceil(listed / resident
                # workgroups) passes, so the per-workgroup rate below is exact only while all listed queries are resident
                case["replay_ms"] = round(ph["replay_ms"], 4)
                case["replay_rows_GBps_all_listed"] = round(ph["listed_queries"] * N * D * 4 / (ph["replay_ms"] * 1e-3) / 1e9, 1)
                case["replay_rows_GBps_per_workgroup_if_one_round"] = round(N * D * 4 / (ph["replay_ms"] * 1e-3) / 1e9, 2)
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
        r.close()
        del rows, queries
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
