"""Method FAST on the multi-device index, on the workload of tools/bench_fast.py (1M sift-like rows, 64 x 4-bit
codes, D = 128, 10 k queries, k = 100): ms per step of the single index (the yardstick, measured in the same
run) and of VaqHipMulti over 2, 4, 8 LOGICAL shards of device 0.  Logical shards share one GPU and cannot
overlap, so no speed-up is to be expected: the figures show what sharding the rows costs on one device -- the
shards' scans one after the other, the exchange (device copies) and the head sort + merge on shard 0.  Every
timed block is repeated (--repeats) and all repeats are printed, so the run-to-run spread can be read off.  Per
leg, one host-entry search gives shard 0's device times (vaqhip_multi_get_info: its own search, the exchange
including the wait for the other shards, head gather + head sort + merge kernel), and the first and last 16
queries are compared slot for slot with tests/fast_ref.py and with the single index.  Prints one JSON line.
Uses bench.build_index; bench.py itself is unchanged.

    python tools/bench_fast_multi.py [--rows 1000000 --nq 10000 --k 100 --steps 5 --warmup 2 --repeats 3]
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
    ap.add_argument("--shards", default="2,4,8")
    ap.add_argument("--learn-ratio", type=float, default=0.1)
    ap.add_argument("--parity-queries", type=int, default=32)
    args = ap.parse_args()
    import fast_ref as fr
    import vaq_amd
    from vaq_amd import harness
    from vaq_amd.index import VaqHipMulti

    dev = torch.device("cuda:0")
    N, k, M = args.rows, args.k, 64
    bits = [4] * M
    queries = harness.sift_like(args.nq, bench.D, stream=7, device=dev)
    heap, host_codes, cents, _ = bench.build_index(bits, N, 0, N, dev, 0, 1, 0, iters=8, keep_host_rows=N)
    eig = heap.mEigenVectors
    heap.close()

    fast = vaq_amd.VaqHipFast(device=0)
    fast.parseMethodString("VAQ256m64min4max4var1,FAST")
    fast.mBitsAlloc = bits
    fast.mCentroidsPerSubs = cents
    fast.mEigenVectors = eig
    fast.mCodebook = host_codes
    train = torch.cat([bench.base_chunk(c, N, dev) for c in range((N + bench.GEN - 1) // bench.GEN)])[:N]
    train = train.cpu().numpy()
    fast.learnQuantization(train, args.learn_ratio)

    res = {"workload": f"FAST {N} rows x {M} x 4-bit, D={bench.D}, {args.nq} queries, k={k}", "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats}
    res["single_ms"], slab, sdis = timed(fast, queries, k, args.steps, args.warmup, args.repeats)
    slab, sdis = slab.cpu().numpy(), sdis.cpu().numpy()

    # parity on the first and the last queries: they lie in the first and the last internal chunk
    P = args.parity_queries
    pick = np.unique(np.concatenate([np.arange(P // 2), np.arange(args.nq - (P - P // 2), args.nq)]))
    lut = fast.build_lut(queries[torch.from_numpy(pick).to(dev)].cpu().numpy())
    el, ed = fr.search_fast(lut, fast.mOffsets, fast.mScale, host_codes, k)

    def parity(lab, dis):
        return int(sum(bool(np.array_equal(lab[p], el[i]) and np.array_equal(dis[p], ed[i])) for i, p in enumerate(pick)))
    res["parity_checked_queries"] = len(pick)
    res["single_parity_ok_queries"] = parity(slab, sdis)
    hq = queries.cpu().numpy()
    for G in [int(x) for x in args.shards.split(",")]:
        m = VaqHipMulti([0] * G, bits, cents, eig)
        moff, msc = m.learn_quantization(train, args.learn_ratio)
        m.set_method(vaq_amd.NNMethod.Fast)
        m.set_codes(host_codes)
        leg = {"quantization_equals_single": bool(np.array_equal(moff, fast.mOffsets) and np.array_equal(msc, fast.mScale))}
        leg["ms"], lab, dis = timed(m, queries, k, args.steps, args.warmup, args.repeats)
        lab, dis = lab.cpu().numpy(), dis.cpu().numpy()
        leg["parity_ok_queries"] = parity(lab, dis)
        leg["equals_single_index_slot_for_slot"] = bool(np.array_equal(lab, slab) and np.array_equal(dis, sdis))
        m.search(hq, k)  # host entry: synchronous, fills the device times of shard 0
        inf = m.info()
        leg["shard0_search_ms"] = round(inf["last_search_ms"], 4)
        leg["exchange_incl_wait_for_other_shards_ms"] = round(inf["last_exchange_ms"], 4)
        leg["head_gather_sort_merge_ms"] = round(inf["last_merge_ms"], 4)
        leg["shard_rows"] = inf["shard_rows"]
        res[f"multi_{G}"] = leg
        m.close()
    print(json.dumps(res), flush=True)
    fast.close()


if __name__ == "__main__":
    main()
