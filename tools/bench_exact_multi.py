"""Option "exact_ties" on the multi-device index, C2 shape (1M sift-like rows x 8 B, 10 k queries, k = 100):
ms per step of the single index with the option on (the yardstick) and off, and of VaqHipMulti over
1, 2, 4, 8 LOGICAL shards of device 0 with the option on and off.  Logical shards share one GPU and
cannot overlap: the figures show what phase A with k + 1, the hand-overs and the extra launches cost,
not a scaling.  Every timed block is repeated (--repeats) and all repeats are printed, so the
run-to-run spread can be read off.  With the option on, the multi result is compared with the single
index's slot for slot.  Prints one JSON line.  Uses bench.build_index; bench.py itself is unchanged.

    python tools/bench_exact_multi.py [--rows 1000000 --nq 10000 --k 100 --steps 5 --warmup 2 --repeats 3]
    --baseline: only the legs that exist without the chain (single on / off, multi off), for runs of an
                older build of the library (VAQHIP_LIB=<path>)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def timed(index, q, k, steps, warmup, repeats):
    nq = q.shape[0]
    lab = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    dis = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    out = []
    for _ in range(repeats):
        for _ in range(warmup):
            index.search_device(q, k, out=(lab, dis))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            index.search_device(q, k, out=(lab, dis))
        e1.record()
        torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1) / steps, 4))
    return out, lab, dis


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    from vaq_amd import harness
    from vaq_amd.index import VaqHipMulti

    dev = torch.device("cuda:0")
    N, k = args.rows, args.k
    bits = [8] * 8
    queries = harness.sift_like(args.nq, bench.D, stream=7, device=dev)
    single, host_codes, cents, _ = bench.build_index(bits, N, 0, N, dev, 0, 1, 0, iters=8, keep_host_rows=N)
    res = {"workload": f"{N} rows x 8 B, D={bench.D}, {args.nq} queries, k={k}", "steps": args.steps,
           "repeats": args.repeats, "baseline_build": bool(args.baseline)}
    res["single_off_ms"], _, _ = timed(single, queries, k, args.steps, args.warmup, args.repeats)
    single.set_option("exact_ties", 1)
    res["single_on_ms"], slab, sdis = timed(single, queries, k, args.steps, args.warmup, args.repeats)
    single.set_option("exact_ties", 0)
    slab, sdis = slab.cpu().numpy(), sdis.cpu().numpy()
    res["queries_replayed_fraction"] = None
    eig = single.mEigenVectors
    for G in [int(x) for x in args.shards.split(",")]:
        m = VaqHipMulti([0] * G, bits, cents, eig)
        m.set_codes(host_codes)
        leg = {}
        leg["off_ms"], _, _ = timed(m, queries, k, args.steps, args.warmup, args.repeats)
        if not args.baseline:
            m.set_option("exact_ties", 1)
            leg["on_ms"], lab, dis = timed(m, queries, k, args.steps, args.warmup, args.repeats)
            lab, dis = lab.cpu().numpy(), dis.cpu().numpy()
            leg["equals_single_index_slot_for_slot"] = bool(
                np.array_equal(lab, slab) and np.array_equal(dis.view(np.uint32), sdis.view(np.uint32)))
        res[f"multi_{G}"] = leg
        m.close()
    # how many queries the flag step lists: equal neighbours among the k + 1 smallest distances
    single.set_option("exact_ties", 0)
    l1, d1 = single.search_device(queries, k + 1)
    torch.cuda.synchronize()
    res["queries_replayed_fraction"] = round(float(((d1[:, 1:] == d1[:, :-1]) & (l1[:, 1:] >= 0)).any(1).float().mean()), 4)
    print(json.dumps(res), flush=True)
    single.close()


if __name__ == "__main__":
    main()
