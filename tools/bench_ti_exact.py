"""Option "exact_ties" on a TI index: what the replay of VAQ::searchTriangleInequality's walk costs against
the default TI path.  C2-shaped codes (1M x 8 x 8-bit), T = 1000 k-means centres over 4 subspaces, 10 k
queries, k = 100, method TI|EA; visit 0.1 and 1, option off and on, and the one-time build of the reference's
member order (the first search with the option set).  Prints one JSON line and writes it to --out.

    python tools/bench_ti_exact.py [--rows 1000000 --nq 10000 --k 100 --clusters 1000 --steps 3 --warmup 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    return e0.elapsed_time(e1) / steps, dis.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ti_exact_1m.json"))
    args = ap.parse_args()
    import vaq_amd
    from vaq_amd.index import NNMethod

    N, k, M, L, seg = args.rows, args.k, 8, 16, 4
    rng = np.random.default_rng(2026)
    cents = [(rng.normal(size=(256, L)) * 20).astype(np.float32) for _ in range(M)]
    codes = rng.integers(0, 256, size=(N, M)).astype(np.uint16)
    X = (rng.normal(size=(args.nq, M * L)) * 20).astype(np.float32)
    v = vaq_amd.VaqHip(device=0)
    v.mBitsAlloc = [8] * M
    v.mCentroidsPerSubs = cents
    v.mMethods = NNMethod.TI | NNMethod.EA
    v.mTISegmentNum = seg
    v.mTIClusterNum = args.clusters
    v.mCodebook = codes
    v.clusterTI(True)  # the k-means of VAQ::clusterTI on the GPU
    q = torch.from_numpy(X).cuda()
    nan_centres = int(np.isnan(np.asarray(v.mTIClusters)).any(1).sum())
    res = {"nan_centres": nan_centres, "workload": f"{N} rows x {M} x 8-bit, T={args.clusters} k-means centres over {seg} subspaces, "
                       f"{args.nq} queries, k={k}, TI|EA"}
    for visit in (0.1, 1.0):
        v.mVisit = visit
        v.set_option("exact_ties", 0)
        off_ms, off_dis = timed(v, q, k, args.steps, args.warmup)
        v.set_option("exact_ties", 1)
        if "member_order_build_ms" not in res:
            t0 = time.perf_counter()
            timed(v, q[:1], k, 1, 0)  # the first search with the option set builds the member order
            res["member_order_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        on_ms, on_dis = timed(v, q, k, args.steps, args.warmup)
        # the stages of one search with the option on: seed_ms is the plan (cluster order), scan_ms the replay
        v.set_option("timing", 1)
        timed(v, q, k, 1, 0)
        tm = v.last_timing()
        v.set_option("timing", 0)
        tag = "visit_%g" % visit
        res[tag] = {"off_ms_per_step": round(off_ms, 3), "exact_ties_ms_per_step": round(on_ms, 3),
                    "ratio": round(on_ms / off_ms, 1),
                    "exact_plan_ms": round(tm["seed_ms"], 3), "exact_replay_ms": round(tm["scan_ms"], 3),
                    "queries_with_equal_distance_lists": int(np.sum(np.all(off_dis == on_dis, axis=1)))}
    v.close()
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
