"""The FAST search method at the paper's Bolt / PQFastScan configuration
(ExperimentsParameters.txt:84-85: 256-bit budget, 64 x 4-bit codes): 1M sift-like
rows, D = 128, 10 k queries, k = 100.  Prints one JSON line: FAST and HEAP ms per
step on the same data and queries, recall@100 of both against exact float ground
truth, the fraction of the int8 matrix-core peak the FAST step reaches, the time
of learnQuantization at ratio 0.1, and how many queries were checked slot for slot
against tests/fast_ref.py (half of them from the end of the batch).  Uses bench.build_index; bench.py itself is unchanged.

    python tools/bench_fast.py [--rows 1000000 --nq 10000 --k 100 --steps 5 --warmup 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

I8_PEAK_OPS = 5.0e15  # dense int8 matrix-core peak of the MI355X, ops/s (2 x its ~2.5 PF BF16 rate)
RECALL_Q = 100


def timed(index, q, k, steps, warmup):
    nq = q.shape[0]
    lab = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    dis = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    for _ in range(warmup):
        index.search_device(q, k, out=(lab, dis))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        index.search_device(q, k, out=(lab, dis))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, lab, dis


def recall(lab, gt_i, k):
    lab = lab[: gt_i.shape[0]].cpu().numpy()
    gt = gt_i.cpu().numpy()
    return float(np.mean([len(set(lab[q].tolist()) & set(gt[q].tolist())) / k for q in range(gt.shape[0])]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--learn-ratio", type=float, default=0.1)
    ap.add_argument("--parity-queries", type=int, default=32)
    args = ap.parse_args()
    import fast_ref as fr
    import vaq_amd
    from vaq_amd import harness

    dev = torch.device("cuda:0")
    N, k, M = args.rows, args.k, 64
    bits = [4] * M
    queries = harness.sift_like(args.nq, bench.D, stream=7, device=dev)
    heap, host_codes, cents, _ = bench.build_index(bits, N, 0, N, dev, 0, 1, 0, iters=8, keep_host_rows=N,
                                                   gt_queries=queries[:RECALL_Q].contiguous(), gt_k=k)
    gt_d, gt_i = bench.build_index.ground_truth

    fast = vaq_amd.VaqHipFast(device=0)
    fast.parseMethodString("VAQ256m64min4max4var1,FAST")
    fast.mBitsAlloc = bits
    fast.mCentroidsPerSubs = cents
    fast.mEigenVectors = heap.mEigenVectors
    fast.mCodebook = host_codes
    train = torch.cat([bench.base_chunk(c, N, dev) for c in range((N + bench.GEN - 1) // bench.GEN)])[:N]
    train = train.cpu().numpy()
    t0 = time.time()
    fast.learnQuantization(train, args.learn_ratio)  # demo_vaq --learn-ratio: XTrain is the dataset
    learn_s = time.time() - t0
    del train

    fast_ms, flab, fdis = timed(fast, queries, k, args.steps, args.warmup)
    heap_ms, hlab, _ = timed(heap, queries, k, args.steps, args.warmup)

    # parity on the first and the last queries: they lie in the first and the last internal chunk
    P = args.parity_queries
    pick = np.unique(np.concatenate([np.arange(P // 2), np.arange(args.nq - (P - P // 2), args.nq)]))
    lut = fast.build_lut(queries[torch.from_numpy(pick).to(dev)].cpu().numpy())
    el, ed = fr.search_fast(lut, fast.mOffsets, fast.mScale, host_codes, k)
    fl, fd = flab.cpu().numpy()[pick], fdis.cpu().numpy()[pick]
    ok = [bool(np.array_equal(fl[i], el[i]) and np.array_equal(fd[i], ed[i])) for i in range(len(pick))]

    n_pad = (N + 31) // 32 * 32
    ops = 2.0 * n_pad * args.nq * 16 * M
    print(json.dumps({
        "workload": f"FAST {N} rows x {M} x 4-bit, D={bench.D}, {args.nq} queries, k={k}",
        "fast_ms_per_step": round(fast_ms, 3),
        "fast_queries_per_s": round(args.nq / (fast_ms / 1e3), 1),
        "heap_ms_per_step": round(heap_ms, 3),
        "fast_recall_at_100": recall(flab, gt_i, k),
        "heap_recall_at_100": recall(hlab, gt_i, k),
        "i8_mfma_peak_fraction": round(ops / (fast_ms / 1e3) / I8_PEAK_OPS, 4),
        "learn_quantization_s": round(learn_s, 2),
        "learn_ratio": args.learn_ratio,
        "parity_checked_queries": len(pick),
        "parity_query_range": [int(pick[0]), int(pick[-1])],
        "parity_ok_queries": int(sum(ok)),
    }), flush=True)
    fast.close()
    heap.close()


if __name__ == "__main__":
    main()
