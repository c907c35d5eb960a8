#!/usr/bin/env python
"""Time the Hamming engine (vaq_amd.VaqBitVec: BitVecEngine::query and ::queryRerank with QueryMethod::Sort) next to
what a user could do before it on the same GPU: a torch formulation of the same top-k (XOR, a gather from a 16-bit
popcount table, a sum, torch.topk), chunked to the same bound on the distance matrix.

  python tools/bench_bitvec.py [--rows 1000000] [--queries 10000] [--k 100] [--bits 128,256] [--factors 2,10]
                               [--reps 5] [--warmup 1] [--out profiles/bitvec_1m.json]

Bits: harness.sign_bits of SIFT-shaped rows (harness.sift_like) projected on their PCA directions, the first n_bits
of them (128 dimensions give 128 bits; 256 bits are those of two independent rotations side by side).  The two routes
are alternated inside one process, each repetition timed with device events around the enqueued calls: median, min
and max of --reps repetitions.  torch.topk orders equal distances its own way, so only the distances of the two
routes are compared before anything is timed, not the labels.  The rerank runs over a byte refiner of the raw rows.

Beside the times: lane_ops = 2 per 32-bit word and pair (one XOR, one BCNT) and the share of 39.3e12 lane-ops/s
 the whole query reaches; the bytes of the distance matrix written and read again.
Not in this tool: a split of the query into scan, head sort and select (the engine has no "timing" option yet), and
vaqhip_search with FAST on the same rows.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VECTOR_RATE = 39.3e12
CHUNK_BYTES = 1 << 30


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 3), "min": round(ms[0], 3), "max": round(ms[-1], 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--bits", default="128,256")
    ap.add_argument("--factors", default="2,10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    import vaq_amd
    from vaq_amd import build, harness
    if not torch.cuda.is_available():
        print("bench_bitvec: no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    N, nq, k = a.rows, a.queries, a.k
    X = harness.sift_like(N, 128, stream=0, device="cuda:0")
    XQ = harness.sift_like(nq, 128, stream=1, device="cuda:0")
    raw8 = X.clamp(0, 255).to(torch.uint8).cpu().numpy()
    XQf = XQ.clamp(0, 255).floor().float().contiguous()
    mean = X.mean(dim=0, keepdim=True)
    E = harness.pca_eigenvectors(X).to(dev)
    planes = [E, E @ harness._rotation(128, 4242, dev)]  # the second 128 bits: the same directions rotated

    def bits_of(M, n_bits):
        P = torch.cat([(M - mean) @ p for p in planes[:(n_bits + 127) // 128]], dim=1)[:, :n_bits]
        return harness.sign_bits(P)

    refiner = vaq_amd.VaqRefiner(128, 0)
    refiner.set_rows_u8(raw8)
    pop16 = torch.tensor([bin(i).count("1") for i in range(65536)], dtype=torch.int16, device=dev)

    def torch_topk(rows16, q16):
        """rows16 int32 [N][4W] (16-bit pieces), q16 int32 [nq][4W] -> (dist int16 [nq][k], idx)"""
        n_pad = (N + 31) // 32 * 32
        chunk = max(1, min(nq, CHUNK_BYTES // 2 // n_pad))
        outs = []
        for q0 in range(0, nq, chunk):
            d = torch.zeros((min(chunk, nq - q0), N), dtype=torch.int16, device=dev)
            for w in range(rows16.shape[1]):
                d += pop16[(q16[q0:q0 + chunk, w, None] ^ rows16[None, :, w])]
            outs.append(torch.topk(d, k, dim=1, largest=False, sorted=True))
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    result = {"rows": N, "queries": nq, "k": k, "reps": a.reps, "source_hash": build.source_hash(),
              "device": torch.cuda.get_device_name(0), "cases": [],
              "not_measured": ["phase split of the query (scan, head sort, select)", "vaqhip_search with FAST on the same rows",
                               "hardware counters", "several GPUs", "1B rows"]}
    for n_bits in [int(b) for b in a.bits.split(",")]:
        rows, queries = bits_of(X, n_bits), bits_of(XQ, n_bits)
        W = rows.shape[1]
        bv = vaq_amd.VaqBitVec(0, n_bits)
        bv.set_rows(rows)
        d_q = torch.from_numpy(queries.view(np.int64)).to(dev)
        out = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
        rows16 = torch.from_numpy(rows.view(np.uint16).astype(np.int32)).to(dev)
        q16 = torch.from_numpy(queries.view(np.uint16).astype(np.int32)).to(dev)
        # the two routes agree on the distances (their labels differ among equal ones)
        bv.query_device(d_q, k, out=out)
        td, _ = torch_topk(rows16, q16)
        torch.cuda.synchronize()
        assert torch.equal(out[1].to(torch.int16), td), "the two routes disagree on the distances"
        ours, theirs = [], []
        for _ in range(a.reps):  # alternated: one repetition of each after its own warm-up
            ours += timed_once(lambda: bv.query_device(d_q, k, out=out), torch, a.warmup if not ours else 0)
            theirs += timed_once(lambda: torch_topk(rows16, q16), torch, a.warmup if not theirs else 0)
        lane_ops = 2.0 * (2 * W) * nq * N
        case = {"n_bits": n_bits, "words": W, "query_ms": stats(ours), "torch_topk_ms": stats(theirs),
                "lane_ops": lane_ops, "vector_rate_share_of_query": round(lane_ops / (stats(ours)["median"] * 1e-3) / VECTOR_RATE, 4),
                "dist_matrix_bytes": 2 * nq * ((N + 31) // 32 * 32), "rerank": []}
        d_oq = XQf.to(dev)
        for factor in [int(f) for f in a.factors.split(",")]:
            if factor * k > 1024:
                continue
            ms = timed(lambda: bv.query_rerank_device(d_q, d_oq, k, factor, refiner, out=out))
            case["rerank"].append({"factor": factor, "query_rerank_ms": stats(ms)})
        result["cases"].append(case)
        bv.close()
        del rows16, q16
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


def timed_once(fn, torch, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return [e0.elapsed_time(e1)]


if __name__ == "__main__":
    sys.exit(main())
