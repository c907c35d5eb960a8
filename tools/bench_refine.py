#!/usr/bin/env python
"""Time the refine stage on resident rows: the resident refiner (vaqhip_refiner_refine_device), the fused call
(vaqhip_search_refine_device) and the earlier entry point (vaqhip_refine_device) on the same rows and candidates.

  python tools/bench_refine.py [--rows 1000000] [--dim 128] [--queries 10000] [--k 100] [--refine 200,1000]
                               [--reps 7] [--warmup 2] [--out profiles/refine_1m.json]

The three are alternated inside one process, each repetition timed with device events around the enqueued call
(`*_ms`: median, with min and max as the spread).  Beside the times: the bytes the candidates imply, nq * R * D * 4,
and that figure over the median time (not a share of peak: many candidates of one query repeat across queries and
come from cache).  `search_ms` is the index's search alone with k = R, so that fused - search can be read off.
The results of the new kernel are checked against each other (fused == search + refine) before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--refine", default="200,1000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exact-ties", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    import vaq_amd
    from vaq_amd import _lib, build
    from helpers import make_case
    if not torch.cuda.is_available():
        print("bench_refine: no GPU: nothing is measured", file=sys.stderr)
        return 1
    L = _lib.load()
    N, D, nq, k = a.rows, a.dim, a.queries, a.k
    c = make_case(2024, D, [8] * 8, N, nq, rotate=False)
    rng = np.random.default_rng(11)
    dev = torch.device("cuda", 0)
    # raw rows: uniform floats, the shape of a float descriptor set (not integer valued)
    rows = torch.empty((N, D), dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    rows.uniform_(0.0, 255.0, generator=g)
    q = torch.from_numpy(c["X"]).to(dev)

    v = vaq_amd.VaqHip()
    v.mBitsAlloc, v.mCentroidsPerSubs, v.mCodebook = c["bits"], c["cents"], c["codes"]
    v._ensure_codes()
    r = vaq_amd.VaqRefiner(D)
    r.set_rows(rows)
    r.exact_ties = bool(a.exact_ties)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    out = {"rows": N, "dim": D, "queries": nq, "k": k, "reps": a.reps, "warmup": a.warmup, "exact_ties": a.exact_ties,
           "device": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "cases": []}
    for R in [int(x) for x in a.refine.split(",")]:
        cand, _ = v.search_device(q, R)
        ol = torch.empty((nq, k), dtype=torch.int32, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        fl, fd = torch.empty_like(ol), torch.empty_like(od)
        sl = torch.empty((nq, R), dtype=torch.int32, device=dev)
        sd = torch.empty((nq, R), dtype=torch.float32, device=dev)

        def new():
            _lib.check(L.vaqhip_refiner_refine_device(r._h, p(q), nq, p(cand), R, k, p(ol), p(od), C.c_void_p(st)))

        def fused():
            _lib.check(L.vaqhip_search_refine_device(v._h, r._h, p(q), nq, R, k, p(fl), p(fd), C.c_void_p(st)))

        def old():
            _lib.check(L.vaqhip_refine_device(0, p(q), nq, D, p(rows), p(cand), R, k, p(ol), p(od), C.c_void_p(st)))

        def search():
            _lib.check(L.vaqhip_search_device(v._h, p(q), nq, R, 0, p(sl), p(sd), C.c_void_p(st)))

        new()
        fused()
        torch.cuda.synchronize()
        assert torch.equal(ol, fl) and torch.equal(od.view(torch.int32), fd.view(torch.int32)), "fused != search + refine"
        calls = {"refiner_refine_device": new, "search_refine_device": fused, "refine_device": old, "search_device": search}
        times = {n: [] for n in calls}
        for it in range(a.warmup + a.reps):
            for n, fn in calls.items():  # alternated: one of each per repetition
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[n].append(e0.elapsed_time(e1))
        cand_bytes = nq * R * D * 4
        case = {"R": R, "candidate_bytes": cand_bytes}
        for n in calls:
            case[n + "_ms"] = stats(times[n])
        for n in ("refiner_refine_device", "refine_device"):
            case[n + "_candidate_GBps"] = round(cand_bytes / (case[n + "_ms"]["median"] * 1e-3) / 1e9, 1)
        case["speedup_vs_refine_device"] = round(case["refine_device_ms"]["median"] / case["refiner_refine_device_ms"]["median"], 3)
        out["cases"].append(case)
        print(json.dumps(case))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    r.close()
    v.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
