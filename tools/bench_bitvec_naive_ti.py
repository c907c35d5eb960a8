#!/usr/bin/env python
"""Time the triangle-inequality form of the Hamming engine's exact queries (VaqBitVec.query_naive_ti_device:
BitVecEngine::queryNaiveTriangleInequality) over a float and over a byte refiner, next to the exhaustive exact search
(VaqRefiner.search_device), which has the same answer, and the exact cluster form (query_naive_clusters_device), whose
recall is bounded by the clusters it visits.

  python tools/bench_bitvec_naive_ti.py [--rows 1000000] [--queries 10000] [--k 100] [--centres 1000] [--atleast 1,8,32]
                                        [--refresh 1,16,64,256,2048] [--reps 5] [--warmup 1]
                                        [--out profiles/bitvec_naive_ti_1m.json]

Rows and centres as tools/bench_bitvec_naive_clusters.py makes them.  All routes alternate inside one process, each
repetition timed with device events around the enqueued call: median, min and max of --reps repetitions.  Beside the
times: evaluated / n (the rows a query loaded, mean and maximum), the build time of set_ti_clusters_from_refiner (a host
clock around the synchronous call), the walk under every --refresh value (option "ti_refresh", float refiner; the
routes above run before the option is touched, at the engine's default), and whether the TI labels equal the exhaustive
search's.
Not in this tool: hardware counters, a split into plan and walk, other T, data with other cluster structure, distinct GPUs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--atleast", default="1,8,32")
    ap.add_argument("--refresh", default="1,16,64,256,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    import vaq_amd
    from bench_bitvec import stats, timed_once
    from vaq_amd import build, harness
    if not torch.cuda.is_available():
        print("bench_bitvec_naive_ti: no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    N, nq, k, T, D = a.rows, a.queries, a.k, a.centres, 128
    X = harness.sift_like(N, D, stream=0, device="cuda:0").contiguous()
    XQ = harness.sift_like(nq, D, stream=1, device="cuda:0").contiguous()
    g = torch.Generator(device="cpu").manual_seed(7)
    cen = X[torch.randperm(N, generator=g)[:T].to(dev)].contiguous().cpu().numpy()

    refiners = {"f32": vaq_amd.VaqRefiner(D, 0), "u8": vaq_amd.VaqRefiner(D, 0)}
    refiners["f32"].set_rows(X)
    refiners["u8"].set_rows_u8(X.to(torch.uint8).contiguous())
    engines, build_ms = {}, {}
    for name, r in refiners.items():  # one engine per refiner: the grouping is the same, the state is per engine
        bv = vaq_amd.VaqBitVec(0, 64)
        bv.set_rows(np.zeros((N, 1), np.uint64))  # the bits are never read
        bv.set_clusters_from_refiner(cen, r)
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bv.set_ti_clusters_from_refiner(cen, r)
            t.append((time.perf_counter() - t0) * 1e3)
        engines[name], build_ms[name] = bv, stats(t)

    def pair():
        return (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
    full, out = pair(), pair()
    ev = torch.zeros(nq, dtype=torch.int64, device=dev)
    result = {"rows": N, "queries": nq, "k": k, "dim": D, "centres": T, "reps": a.reps, "source_hash": build.source_hash(),
              "device": torch.cuda.get_device_name(0), "set_ti_clusters_from_refiner_ms": build_ms,
              "not_measured": ["hardware counters", "split into plan and walk", "other T", "data with other cluster structure",
                               "distinct GPUs: one device, one process, one run of this tool"]}
    refiners["f32"].search_device(XQ, k, out=full)
    for name in refiners:
        engines[name].query_naive_ti_device(XQ, k, refiners[name], out=out, evaluated_out=ev)
        torch.cuda.synchronize()
        frac = ev.double() / N
        result["ti_" + name] = {"evaluated_over_n": {"mean": round(float(frac.mean()), 5), "max": round(float(frac.max()), 5)},
                                "labels_equal_exhaustive": bool((out[0] == full[0]).all()),
                                "distances_equal_sqrt_exhaustive": bool((out[1] == full[1].sqrt()).all())}

    routes = {"exhaustive": lambda: refiners["f32"].search_device(XQ, k, out=full)}
    for name in refiners:
        routes["ti_" + name] = lambda name=name: engines[name].query_naive_ti_device(XQ, k, refiners[name], out=out)
    for atleast in [int(x) for x in a.atleast.split(",")]:
        routes["naive_clusters_f32_atleast_%d" % atleast] = lambda atleast=atleast: engines["f32"].query_naive_clusters_device(
            XQ, k, refiners["f32"], atleast_cluster=atleast, out=out)
    ms = {name: [] for name in routes}
    for _ in range(a.reps):  # alternated: one repetition of each after its own warm-up
        for name, run in routes.items():
            ms[name] += timed_once(run, torch, a.warmup if not ms[name] else 0)
    for name, t in ms.items():
        if name.startswith("ti_"):
            result[name]["ms"] = stats(t)
        else:
            result[name + "_ms"] = stats(t)

    # the threshold-refresh policies: the float refiner's walk under each value, alternated
    values = [int(x) for x in a.refresh.split(",")]
    pol = {v: [] for v in values}
    bv = engines["f32"]
    for _ in range(a.reps):
        for v in values:
            bv.set_option("ti_refresh", v)
            pol[v] += timed_once(lambda: bv.query_naive_ti_device(XQ, k, refiners["f32"], out=out, evaluated_out=ev), torch,
                                 a.warmup if not pol[v] else 0)
    result["ti_refresh_policies_f32"] = []
    for v in values:
        bv.set_option("ti_refresh", v)
        bv.query_naive_ti_device(XQ, k, refiners["f32"], out=out, evaluated_out=ev)
        torch.cuda.synchronize()
        result["ti_refresh_policies_f32"].append({"ti_refresh": v, "ms": stats(pol[v]),
                                                  "evaluated_over_n_mean": round(float((ev.double() / N).mean()), 5)})
    for r in refiners.values():
        r.close()
    for bv in engines.values():
        bv.close()
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
