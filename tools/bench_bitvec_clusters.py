#!/usr/bin/env python
"""Time the cluster form of the Hamming engine (VaqBitVec.query_clusters_device: BitVecEngine::queryWithClusterInfo
with QueryMethod::Sort) next to the exhaustive form (query_device) over the same rows.

  python tools/bench_bitvec_clusters.py [--rows 1000000] [--queries 10000] [--k 100] [--bits 128,256]
                                        [--centres 1000] [--atleast 1,8,32] [--reps 5] [--warmup 1]
                                        [--out profiles/bitvec_clusters_1m.json]

Bits as tools/bench_bitvec.py makes them: harness.sign_bits of SIFT-shaped rows projected on their PCA directions.
The centres are rows sampled from the raw data; every row goes to its nearest centre (torch).  The two routes are
alternated inside one process, each repetition timed with device events around the enqueued call: median, min and
max of --reps repetitions.

Beside the times: the mean number of candidates per query (C_q) and the share of queries whose centre distances hold
an equal pair (they take the plan's one-thread std::sort) -- both worked out in torch from its own centre distances,
whose summation order is not the kernel's, so they are estimates; and recall@k against the exhaustive form counted on
distances: a slot counts when its distance is at most the exhaustive answer's k-th.
Not in this tool: a split into plan and select, hardware counters, the rerank form.
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
    ap.add_argument("--bits", default="128,256")
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--atleast", default="1,8,32")
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
        print("bench_bitvec_clusters: no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    N, nq, k, T = a.rows, a.queries, a.k, a.centres
    X = harness.sift_like(N, 128, stream=0, device="cuda:0")
    XQ = harness.sift_like(nq, 128, stream=1, device="cuda:0").contiguous()
    mean = X.mean(dim=0, keepdim=True)
    E = harness.pca_eigenvectors(X).to(dev)
    planes = [E, E @ harness._rotation(128, 4242, dev)]

    def bits_of(M, n_bits):
        P = torch.cat([(M - mean) @ p for p in planes[:(n_bits + 127) // 128]], dim=1)[:, :n_bits]
        return harness.sign_bits(P)

    g = torch.Generator(device="cpu").manual_seed(7)
    cen = X[torch.randperm(N, generator=g)[:T].to(dev)].contiguous()
    idx = torch.cat([torch.cdist(X[r0:r0 + 65536], cen).argmin(dim=1) for r0 in range(0, N, 65536)]).to(torch.int32)
    sizes = torch.bincount(idx.long(), minlength=T)
    d_cen = torch.cdist(XQ, cen) ** 2
    d_sorted, order = torch.sort(d_cen, dim=1, stable=True)
    cum = sizes[order].cumsum(dim=1)
    first = (cum >= k).float().argmax(dim=1) + 1  # centres walked until k rows are met
    tie_share = float((d_sorted[:, 1:] == d_sorted[:, :-1]).any(dim=1).float().mean())

    result = {"rows": N, "queries": nq, "k": k, "centres": T, "reps": a.reps, "source_hash": build.source_hash(),
              "device": torch.cuda.get_device_name(0), "cluster_rows": {"min": int(sizes.min()), "max": int(sizes.max())},
              "std_sort_fallback_share_estimate": round(tie_share, 5), "cases": [],
              "not_measured": ["split into plan and select", "hardware counters (L2 hits of pass B)", "the rerank form"]}
    for n_bits in [int(b) for b in a.bits.split(",")]:
        rows, queries = bits_of(X, n_bits), bits_of(XQ, n_bits)
        bv = vaq_amd.VaqBitVec(0, n_bits)
        bv.set_rows(rows)
        bv.set_clusters(cen.cpu().numpy(), idx.cpu().numpy())
        d_q = torch.from_numpy(queries.view(np.int64)).to(dev)
        full = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
        out = (torch.empty_like(full[0]), torch.empty_like(full[1]))
        bv.query_device(d_q, k, out=full)
        case = {"n_bits": n_bits, "words": rows.shape[1], "atleast": []}
        everything = []
        for atleast in [int(x) for x in a.atleast.split(",")]:
            run = lambda: bv.query_clusters_device(d_q, XQ, k, atleast_cluster=atleast, out=out)  # noqa: E731
            run()
            torch.cuda.synchronize()
            hit = ((out[1] <= full[1][:, k - 1:k]) & (out[0] >= 0)).float().sum(dim=1) / k
            visit = torch.clamp(first, min=atleast)
            c_q = cum.gather(1, (visit - 1)[:, None]).float().mean()
            ours, theirs = [], []
            for _ in range(a.reps):  # alternated: one repetition of each after its own warm-up
                ours += timed_once(run, torch, a.warmup if not ours else 0)
                theirs += timed_once(lambda: bv.query_device(d_q, k, out=full), torch, a.warmup if not theirs else 0)
            everything += theirs
            case["atleast"].append({"atleast_cluster": atleast, "query_clusters_ms": stats(ours), "mean_candidates_estimate": round(float(c_q), 1),
                                    "recall_at_k_on_distances": round(float(hit.mean()), 4)})
        case["query_ms"] = stats(everything)
        result["cases"].append(case)
        bv.close()
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
