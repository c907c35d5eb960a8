"""Option "exact_ties" on a sequential-sum (BitVecEngine::queryLUT) index: what the replay under the std
heap costs.  D = M = 32 scalar quantisers of 4 bits, 1M rows, 1024 queries, k = 100; a fraction of the rows
are copies of other rows, so that most queries have equal distances inside their top k + 1 and are replayed.
Prints one JSON line: ms per step with the option off and on, how many queries had ties (were replayed),
and how many of the checked queries equal tests/seq_exact_ref.py's restatement slot for slot.

    python tools/bench_seq_exact.py [--rows 1000000 --nq 1024 --k 100 --steps 5 --warmup 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


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
    return e0.elapsed_time(e1) / steps, lab.cpu().numpy(), dis.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dup-frac", type=float, default=0.3)
    ap.add_argument("--parity-queries", type=int, default=4)
    args = ap.parse_args()
    import seq_exact_ref as sr
    import vaq_amd

    N, k, M, B = args.rows, args.k, 32, 4
    rng = np.random.default_rng(2025)
    bits = [B] * M
    cent = np.zeros((256, M), np.float32)
    for d in range(M):
        cent[: 1 << B, d] = np.sort(rng.normal(size=1 << B) * 20).astype(np.float32)
    codes = rng.integers(0, 1 << B, size=(N, M)).astype(np.uint16)
    ndup = int(args.dup_frac * N)
    codes[rng.integers(0, N, ndup)] = codes[rng.integers(0, N, ndup)]
    X = (rng.normal(size=(args.nq, M)) * 20).astype(np.float32)

    v = vaq_amd.VaqHip(device=0, sequential_sum=True)
    v.mBitsAlloc = bits
    v.mCentroidsPerSubs = sr.centroid_list(bits, cent)
    v.mCodebook = codes
    q = torch.from_numpy(X).cuda()
    off_ms, _, off_dis = timed(v, q, k, args.steps, args.warmup)
    v.set_option("exact_ties", 1)
    on_ms, on_lab, on_dis = timed(v, q, k, args.steps, args.warmup)
    # replayed: equal neighbours among the k + 1 smallest distances
    _, _, d1 = timed(v, q, k + 1, 1, 0)
    tied = int(np.sum(np.any(np.diff(d1, axis=1) == 0, axis=1)))
    ok = 0
    for i in range(min(args.parity_queries, args.nq)):
        lab, dis = sr.query_lut_topk(sr.row_dists(X[i], bits, cent, codes), k)
        ok += int(np.array_equal(lab, on_lab[i]) and np.array_equal(dis.view(np.uint32), on_dis[i].view(np.uint32)))
    print(json.dumps({
        "workload": f"queryLUT sum, {N} rows x {M} x {B}-bit, {args.nq} queries, k={k}, dup_frac={args.dup_frac}",
        "off_ms_per_step": round(off_ms, 3),
        "exact_ties_ms_per_step": round(on_ms, 3),
        "queries_replayed": tied,
        "distances_equal_off_and_on": bool(np.array_equal(off_dis.view(np.uint32), on_dis.view(np.uint32))),
        "parity_checked_queries": min(args.parity_queries, args.nq),
        "parity_ok_queries": ok,
    }), flush=True)
    v.close()


if __name__ == "__main__":
    main()
