#!/usr/bin/env python
"""Time the cluster index (VaqRefiner.cluster_index_device: computeClusterIndex on the device) over a float and over a
byte refiner, next to a torch formulation on the same device, and VaqBitVec.set_clusters_from_refiner next to
set_clusters with a precomputed index.

  python tools/bench_cluster_index.py [--rows 1000000] [--centres 1000] [--reps 5] [--warmup 1]
                                      [--out profiles/cluster_index_1m.json]

Rows and centres as tools/bench_bitvec_clusters.py makes them (1M x 128 byte-valued rows, the centres sampled from the
rows).  The three routes are alternated inside one process, each repetition timed with device events around the
enqueued call and waited for: median, min and max of --reps repetitions.  The yardstick is |x|^2 - 2 x c^T + |c|^2 by
fp32 matmul in row chunks whose distance block stays within 1 GiB, then argmin: it uses the matrix units and reorders
the sum, so its index may differ; the rows where it does are counted.  The share of the bound is the median over
3 n T D lane operations at the fp32 vector rate of the README (39.3 T lane-ops/s): the vector rate is the bound taken.
The set_clusters pair is timed with the host clock, three repetitions each.
Not in this tool: hardware counters, the kernel time from a trace (the events surround one enqueued kernel).
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
VECTOR_LANE_OPS_PER_S = 39.3e12


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--centres", type=int, default=1000)
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
        print("bench_cluster_index: no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    N, T, D = a.rows, a.centres, 128
    X = harness.sift_like(N, D, stream=0, device="cuda:0").contiguous()
    g = torch.Generator(device="cpu").manual_seed(7)
    cen = X[torch.randperm(N, generator=g)[:T].to(dev)].contiguous()
    refiners = {"f32": vaq_amd.VaqRefiner(D, 0), "u8": vaq_amd.VaqRefiner(D, 0)}
    refiners["f32"].set_rows(X)
    refiners["u8"].set_rows_u8(X.to(torch.uint8).contiguous())
    chunk = max(1, (1 << 30) // (4 * T))
    c2 = (cen * cen).sum(dim=1)[None]
    answers = {}

    def torch_route():
        answers["torch"] = torch.cat([((x * x).sum(dim=1, keepdim=True) - 2.0 * (x @ cen.T) + c2).argmin(dim=1)
                                      for x in X.split(chunk)]).to(torch.int32)

    def ours(name):
        def run():
            answers[name] = refiners[name].cluster_index_device(cen)
        return run
    routes = {"f32": ours("f32"), "u8": ours("u8"), "torch": torch_route}
    ms = {name: [] for name in routes}
    for _ in range(a.reps):  # alternated: one repetition of each after its own warm-up
        for name, run in routes.items():
            ms[name] += timed_once(run, torch, a.warmup if not ms[name] else 0)
    bound_ms = 3.0 * N * T * D / VECTOR_LANE_OPS_PER_S * 1e3
    result = {"rows": N, "dim": D, "centres": T, "reps": a.reps, "source_hash": build.source_hash(),
              "device": torch.cuda.get_device_name(0), "vector_bound_ms": round(bound_ms, 3),
              "bound_taken": "3 n T D lane operations at 39.3 T lane-ops/s (fp32 vector rate)",
              "f32_equals_u8": bool(torch.equal(answers["f32"], answers["u8"])),
              "rows_unassigned": int((answers["f32"] < 0).sum()),
              "torch_rows_differing": int((answers["torch"] != answers["f32"]).sum())}
    for name, t in ms.items():
        result[name + "_ms"] = stats(t)
    for name in ("f32", "u8"):
        result[name + "_share_of_vector_bound"] = round(bound_ms / result[name + "_ms"]["median"], 3)

    # with and without: the cluster state from the refiner, and from an index the caller already has
    bv = vaq_amd.VaqBitVec(0, D)
    bv.set_rows(harness.sign_bits(X - X.mean(dim=0, keepdim=True)))
    cen_h = cen.cpu().numpy()
    idx_h = answers["f32"].cpu().numpy()
    host = {"assign_and_fetch": lambda: refiners["f32"].cluster_index(cen_h),
            "set_clusters_from_refiner": lambda: bv.set_clusters_from_refiner(cen_h, refiners["f32"]),
            "set_clusters_precomputed": lambda: bv.set_clusters(cen_h, idx_h)}
    for name, run in host.items():
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            t.append((time.perf_counter() - t0) * 1e3)
        result[name + "_host_ms"] = stats(t)
    result["not_measured"] = ["hardware counters", "kernel time from a trace (the events surround one enqueued kernel)",
                              "the scalar-operand form of the centre values", "two rows a lane, other TC / DC",
                              "distinct GPUs: one device, one process, one run of this tool"]
    for r in refiners.values():
        r.close()
    bv.close()
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
