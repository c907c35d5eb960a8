#!/usr/bin/env python
"""Time VaqRefiner.fit_centres (KMeans::fit on the device) over a float and over a byte refiner, per iteration and split
into its phases, next to the only route to the same centres without it: the cluster index on the device for the assign,
then the index fetched and the centres updated on the host.

  python tools/bench_fit_centres.py [--rows 1000000] [--centres 1000] [--iters 4] [--reps 5] [--warmup 1]
                                    [--out profiles/fit_centres_1m.json]

Rows as tools/bench_cluster_index.py makes them (1M x 128 byte-valued rows), the seeds a seeded permutation's head.  A
repetition is one fit of --iters iterations (max_iter = --iters; byte-valued rows do not converge that early) timed with
the host clock around the synchronous call; the phases are the library's own device events, summed over the iterations
and divided by them.  Route (a) is timed in the same process, alternated with the fits: one iteration = the assign
(cluster_index_device, events) + the fetch of the index and a host update (a stable argsort by centre, then
np.add.reduceat over the sorted float32 rows and a division; host clock).  Its sums are numpy's, not the reference's
order.  Median, min and max of --reps repetitions.
Not in this tool: route (b), the km_* Lloyd iteration of the TI k-means (it is reached only through an index's decoded
codes and samples at most max(256 k, 65536) rows); hardware counters; kernel times from a trace; the update kernel at a
skewed assignment or at D = 8176.
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
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=4)
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
        print("bench_fit_centres: no GPU: nothing is measured", file=sys.stderr)
        return 1
    N, T, D = a.rows, a.centres, 128
    X = harness.sift_like(N, D, stream=0, device="cuda:0").contiguous()
    X_h = X.cpu().numpy()
    seeds = np.random.RandomState(7).permutation(N)[:T].astype(np.int32)
    refiners = {"f32": vaq_amd.VaqRefiner(D, 0), "u8": vaq_amd.VaqRefiner(D, 0)}
    refiners["f32"].set_rows(X)
    refiners["u8"].set_rows_u8(X.to(torch.uint8).contiguous())
    cen = X[torch.from_numpy(seeds.astype(np.int64)).cuda()].contiguous()
    ms = {k: [] for k in ("f32_fit", "u8_fit", "f32_assign", "f32_group", "f32_update", "u8_assign", "u8_group", "u8_update",
                          "a_assign", "a_fetch_and_host_update")}
    answers, idx = {}, {}

    def route_a_assign():
        idx["d"] = refiners["f32"].cluster_index_device(cen)

    for rep in range(a.reps + a.warmup):  # alternated; the first --warmup rounds are dropped
        keep = rep >= a.warmup
        for name, r in refiners.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            answers[name] = r.fit_centres(T, seeds, a.iters)
            wall = (time.perf_counter() - t0) * 1e3
            t = r.last_fit_centres_timing()
            if keep:
                ms[name + "_fit"].append(wall / t["iterations"])
                for p in ("assign", "group", "update"):
                    ms[name + "_" + p].append(t[p + "_ms"] / t["iterations"])
        assign = timed_once(route_a_assign, torch, 0)
        t0 = time.perf_counter()
        idx_h = idx["d"].cpu().numpy()
        order = np.argsort(idx_h, kind="stable")
        present, first = np.unique(idx_h[order], return_index=True)
        new = np.full((T, D), np.nan, np.float32)
        new[present] = np.add.reduceat(X_h[order], first, axis=0) / np.diff(np.append(first, N)).astype(np.float32)[:, None]
        host = (time.perf_counter() - t0) * 1e3
        if keep:
            ms["a_assign"] += assign
            ms["a_fetch_and_host_update"].append(host)
    result = {"rows": N, "dim": D, "centres": T, "iterations_per_fit": a.iters, "reps": a.reps,
              "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
              "f32_equals_u8": all(np.array_equal(x, y, equal_nan=True) for x, y in zip(answers["f32"][:2], answers["u8"][:2])),
              "empty_centres": int(np.isnan(answers["f32"][0][:, 0]).sum()),
              "largest_cluster_rows": int(np.bincount(answers["f32"][1], minlength=T).max())}
    for name, t in ms.items():
        result[name + "_ms_per_iteration"] = stats(t)
    a_iter = result["a_assign_ms_per_iteration"]["median"] + result["a_fetch_and_host_update_ms_per_iteration"]["median"]
    result["route_a_ms_per_iteration_median_sum"] = round(a_iter, 3)
    result["route_a_over_f32_fit"] = round(a_iter / result["f32_fit_ms_per_iteration"]["median"], 2)
    result["not_measured"] = ["route (b): the km_* Lloyd iteration (reached only through an index's decoded codes, sampled)",
                              "hardware counters", "kernel times from a trace", "the update kernel at a skewed assignment",
                              "the update kernel at D = 8176, T = 16", "distinct GPUs: one device, one process, one run of this tool"]
    for r in refiners.values():
        r.close()
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
