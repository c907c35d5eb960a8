"""The multi-device refiner (VaqMultiRefiner) next to the single refiner on the same rows and candidates.

    python tools/bench_refine_multi.py --out profiles/refine_multi_1m.json

Workload: 1M x 128 float rows, 10 000 queries, k = 100, R = 200 and R = 1000 (--exact-ties 1: with the one-thread
heap replay in the selection).
G = 1, 2, 4, 8 shards over distinct GPUs where the machine has that many, logical shards on GPU 0 otherwise -- the
file says which.  Device events, median of seven, the two refiners alternating in one process.  The four phases
(broadcast, distances, gather, select) are the refiner's own events (option "timing"); `total_ms` is measured around
the whole call on the caller's stream.  Nothing is fixed in advance: the file holds what was measured."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--R", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--shards", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--exact-ties", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_multi_1m.json"))
    a = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import build
    n_gpus = torch.cuda.device_count()
    rng = np.random.default_rng(11)
    Xt = rng.uniform(0, 255, size=(a.rows, a.dim)).astype(np.float32)
    Xq = rng.uniform(0, 255, size=(a.nq, a.dim)).astype(np.float32)
    torch.cuda.set_device(0)
    dq = torch.from_numpy(Xq).cuda()
    one = vaq_amd.VaqRefiner(a.dim, device=0)
    one.set_rows(Xt)
    one.exact_ties = bool(a.exact_ties)
    res = dict(tool="tools/bench_refine_multi.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0),
               gpus=n_gpus, rows=a.rows, dim=a.dim, nq=a.nq, k=a.k, exact_ties=a.exact_ties, repeats=a.repeats,
               timing="device events, median of %d, single and multi alternating in one process" % a.repeats, runs=[])
    for R in a.R:
        dl = torch.from_numpy(rng.integers(0, a.rows, size=(a.nq, R)).astype(np.int32)).cuda()
        out1 = (torch.empty((a.nq, a.k), dtype=torch.int32, device="cuda:0"), torch.empty((a.nq, a.k), device="cuda:0"))
        outm = (torch.empty_like(out1[0]), torch.empty_like(out1[1]))
        for G in a.shards:
            distinct = n_gpus >= G
            devices = list(range(G)) if distinct else [0] * G
            m = vaq_amd.VaqMultiRefiner(devices, a.dim)
            m.set_rows(Xt)
            m.exact_ties = bool(a.exact_ties)
            m.set_option("timing", 1)
            for _ in range(2):
                one.refine_device(dq, dl, a.k, out=out1)
                m.refine_device(dq, dl, a.k, out=outm)
            torch.cuda.synchronize()
            assert torch.equal(out1[0], outm[0]) and torch.equal(out1[1].view(torch.int32), outm[1].view(torch.int32))
            t1, tm, ph = [], [], []
            for _ in range(a.repeats):
                t1.append(timed(lambda: one.refine_device(dq, dl, a.k, out=out1), torch))
                tm.append(timed(lambda: m.refine_device(dq, dl, a.k, out=outm), torch))
                inf = m.info()
                ph.append([inf[f"last_{p}_ms"] for p in ("broadcast", "distances", "gather", "select")])
            med = lambda v: round(statistics.median(v), 4)
            phm = [med([p[i] for p in ph]) for i in range(4)]
            run = dict(R=R, shards=G, placement="distinct GPUs" if distinct else "logical shards on GPU 0",
                       single_ms=med(t1), single_min_ms=round(min(t1), 4), single_max_ms=round(max(t1), 4),
                       total_ms=med(tm), total_min_ms=round(min(tm), 4), total_max_ms=round(max(tm), 4),
                       broadcast_ms=phm[0], distances_ms=phm[1], gather_ms=phm[2], select_ms=phm[3],
                       gathered_bytes=(G - 1) * a.nq * R * 4, broadcast_bytes_per_shard=a.nq * (a.dim + R) * 4)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            m.close()
    one.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
