#!/usr/bin/env python
"""Time the exact cluster form of the Hamming engine (VaqBitVec.query_naive_clusters_device:
BitVecEngine::queryNaiveWithClusterInfo with QueryMethod::Sort) over a float and over a byte refiner, next to the bit
route over the same visit (query_rerank_clusters_device, factor 10) and the exhaustive exact search
(VaqRefiner.search_device) over the same rows.

  python tools/bench_bitvec_naive_clusters.py [--rows 1000000] [--queries 10000] [--k 100] [--bits 128] [--centres 1000]
                                              [--atleast 1,8,32] [--factor 10] [--reps 5] [--warmup 1]
                                              [--out profiles/bitvec_naive_clusters_1m.json]

Rows, bits, centres and cluster indices as tools/bench_bitvec_clusters.py makes them.  The four routes are alternated
inside one process, each repetition timed with device events around the enqueued call: median, min and max of --reps
repetitions.  recall@k of each route is counted on distances against the exhaustive answer: a slot counts when its
distance is at most the exhaustive k-th.  Beside the times: the bytes of raw rows the mean candidate count implies
(derived from torch's own centre distances, an estimate) over the median time.
Not in this tool: hardware counters, how often the pool is compacted, a split into plan and select, distinct GPUs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--bits", type=int, default=128)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--atleast", default="1,8,32")
    ap.add_argument("--factor", type=int, default=10)
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
        print("bench_bitvec_naive_clusters: no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    N, nq, k, T, D = a.rows, a.queries, a.k, a.centres, 128
    X = harness.sift_like(N, D, stream=0, device="cuda:0").contiguous()
    XQ = harness.sift_like(nq, D, stream=1, device="cuda:0").contiguous()
    mean = X.mean(dim=0, keepdim=True)
    E = harness.pca_eigenvectors(X).to(dev)
    planes = [E, E @ harness._rotation(D, 4242, dev)]

    def bits_of(M):
        P = torch.cat([(M - mean) @ p for p in planes[:(a.bits + 127) // 128]], dim=1)[:, :a.bits]
        return harness.sign_bits(P)

    g = torch.Generator(device="cpu").manual_seed(7)
    cen = X[torch.randperm(N, generator=g)[:T].to(dev)].contiguous()
    idx = torch.cat([torch.cdist(X[r0:r0 + 65536], cen).argmin(dim=1) for r0 in range(0, N, 65536)]).to(torch.int32)
    sizes = torch.bincount(idx.long(), minlength=T)
    order = torch.sort(torch.cdist(XQ, cen) ** 2, dim=1, stable=True)[1]
    cum = sizes[order].cumsum(dim=1)
    first = (cum >= k).float().argmax(dim=1) + 1  # centres walked until k rows are met

    bv = vaq_amd.VaqBitVec(0, a.bits)
    bv.set_rows(bits_of(X))
    bv.set_clusters(cen.cpu().numpy(), idx.cpu().numpy())
    d_q = torch.from_numpy(bits_of(XQ).view(np.int64)).to(dev)
    refiners = {"f32": vaq_amd.VaqRefiner(D, 0), "u8": vaq_amd.VaqRefiner(D, 0)}
    refiners["f32"].set_rows(X)
    refiners["u8"].set_rows_u8(X.to(torch.uint8).contiguous())

    def pair():
        return (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
    full, out = pair(), pair()
    refiners["f32"].search_device(XQ, k, out=full)
    result = {"rows": N, "queries": nq, "k": k, "dim": D, "centres": T, "n_bits": a.bits, "rerank_factor": a.factor,
              "reps": a.reps, "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
              "cluster_rows": {"min": int(sizes.min()), "max": int(sizes.max())}, "atleast": [],
              "not_measured": ["hardware counters", "how often the pool is compacted", "split into plan and select",
                               "distinct GPUs: one device, one process, one run of this tool"]}
    everything = []
    for atleast in [int(x) for x in a.atleast.split(",")]:
        routes = {
            "naive_f32": lambda: bv.query_naive_clusters_device(XQ, k, refiners["f32"], atleast_cluster=atleast, out=out),
            "naive_u8": lambda: bv.query_naive_clusters_device(XQ, k, refiners["u8"], atleast_cluster=atleast, out=out),
            "rerank_clusters": lambda: bv.query_rerank_clusters_device(d_q, XQ, k, a.factor, refiners["f32"],
                                                                       atleast_cluster=atleast, out=out),
            "exhaustive": lambda: refiners["f32"].search_device(XQ, k, out=full),
        }
        c_q = float(cum.gather(1, (torch.clamp(first, min=atleast) - 1)[:, None]).float().mean())
        entry = {"atleast_cluster": atleast, "mean_candidates_estimate": round(c_q, 1)}
        ms = {name: [] for name in routes}
        for name, run in routes.items():
            if name == "exhaustive":
                continue
            run()
            torch.cuda.synchronize()
            hit = ((out[1] <= full[1][:, k - 1:k]) & (out[0] >= 0)).float().sum(dim=1) / k
            entry["recall_at_k_" + name] = round(float(hit.mean()), 4)
        for _ in range(a.reps):  # alternated: one repetition of each after its own warm-up
            for name, run in routes.items():
                ms[name] += timed_once(run, torch, a.warmup if not ms[name] else 0)
        everything += ms.pop("exhaustive")
        for name, t in ms.items():
            entry[name + "_ms"] = stats(t)
        for name, elem in (("naive_f32", 4), ("naive_u8", 1)):  # the raw rows' bytes a step reads, from the estimate
            entry[name + "_row_gb_per_s_estimate"] = round(c_q * D * elem * nq / entry[name + "_ms"]["median"] / 1e6, 1)
        result["atleast"].append(entry)
    result["exhaustive_ms"] = stats(everything)
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
