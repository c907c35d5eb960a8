#!/usr/bin/env python
"""Time the resident refiner over BYTE rows (vaqhip_refiner_set_rows_u8) against the float refiner of the same build
over the same rows widened: the refine (vaqhip_refiner_refine_device) and the exhaustive form
(vaqhip_refiner_search_device).

  python tools/bench_refine_u8.py [--rows 1000000] [--dim 128] [--queries 10000] [--k 100] [--refine 200,1000]
                                  [--exhaustive 100,10000] [--reps 5] [--warmup 2] [--out profiles/refine_u8_1m.json]

Rows are harness.sift_like (integer-valued in [0, 255], SIFT-shaped) cast to uint8 -- the cast is checked to be
lossless -- and the queries are sift_like plus a fraction, so that they are not byte-valued.  The candidates of the
refine legs are each query's R nearest rows (the exhaustive form's answer with k = R), shuffled per query: the rows a
good index returns, in no particular order.  Per leg the float and the byte refiner are alternated inside one process,
each repetition timed with device events around the enqueued call (median, min, max), and after EVERY repetition the
two answers are compared, labels and distance bits.  Beside the times: the resident row bytes of each form (what was
allocated, N * D * element size) and the bytes the candidates imply (nq * R * D * element size; not what the memory
system moved: candidates repeat across queries and come from cache).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def verdict(f32, u8):
    """how the byte form's range lies against the float form's"""
    if u8["max"] < f32["min"]:
        return "faster beyond the spread"
    if u8["min"] > f32["max"]:
        return "slower beyond the spread"
    return "within the spread"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--refine", default="200,1000")
    ap.add_argument("--exhaustive", default="100,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    import vaq_amd
    from vaq_amd import _lib, build, harness
    if not torch.cuda.is_available():
        print("bench_refine_u8: no GPU: nothing is measured", file=sys.stderr)
        return 1
    if a.reps < 5:
        print("bench_refine_u8: at least five repeats", file=sys.stderr)
        return 2
    L = _lib.load()
    N, D, k, nq = a.rows, a.dim, a.k, a.queries
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())

    rows_f = harness.sift_like(N, D, stream=0, device=dev)
    rows_8 = rows_f.to(torch.uint8)
    assert torch.equal(rows_8.float(), rows_f), "the rows are not byte-valued"
    g = torch.Generator(device=dev).manual_seed(23)
    nq_all = max([nq] + [int(x) for x in a.exhaustive.split(",")])
    queries = harness.sift_like(nq_all, D, stream=1, device=dev) + torch.rand((nq_all, D), generator=g, device=dev)
    rf, r8 = vaq_amd.VaqRefiner(D), vaq_amd.VaqRefiner(D)
    rf.set_rows(rows_f)
    r8.set_rows_u8(rows_8)
    del rows_f, rows_8
    torch.cuda.empty_cache()
    assert rf.elem_size == 4 and r8.elem_size == 1
    refiners = {"f32": rf, "u8": r8}
    out = {"rows": N, "dim": D, "k": k, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "source_hash": build.source_hash(),
           "resident_row_bytes": {"f32": N * D * 4, "u8": N * D}, "shards": "one device, no shards", "cases": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run_leg(case, calls, outs):
        """calls / outs: per form the enqueue and its (labels, distances); alternated, compared on every repetition"""
        times = {n: [] for n in calls}
        for it in range(a.warmup + a.reps):
            for n, fn in calls.items():
                ms = timed(fn)
                if it >= a.warmup:
                    times[n].append(ms)
            same = torch.equal(outs["f32"][0], outs["u8"][0]) and torch.equal(outs["f32"][1].view(torch.int32),
                                                                              outs["u8"][1].view(torch.int32))
            assert same, f"{case}: the byte refiner's answer differs from the float refiner's (repetition {it})"
        for n in calls:
            case[n + "_ms"] = stats(times[n])
        case["results_equal_on_every_repeat"] = True
        case["u8_over_f32_median"] = round(case["u8_ms"]["median"] / case["f32_ms"]["median"], 4)
        case["u8_vs_f32"] = verdict(case["f32_ms"], case["u8_ms"])
        out["cases"].append(case)
        print(json.dumps(case), flush=True)

    q = queries[:nq].contiguous()
    for R in [int(x) for x in a.refine.split(",")]:
        near, _ = rf.search_device(q, R)
        perm = torch.rand((nq, R), generator=g, device=dev).argsort(dim=1)
        cand = torch.gather(near, 1, perm).contiguous()
        del near, perm
        calls, outs = {}, {}
        for n, r in refiners.items():
            ol = torch.empty((nq, k), dtype=torch.int32, device=dev)
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)
            outs[n] = (ol, od)
            calls[n] = (lambda r=r, ol=ol, od=od: _lib.check(L.vaqhip_refiner_refine_device(
                r._h, p(q), nq, p(cand), R, k, p(ol), p(od), C.c_void_p(st))))
        run_leg({"call": "refine", "queries": nq, "R": R,
                 "candidate_bytes": {"f32": nq * R * D * 4, "u8": nq * R * D}}, calls, outs)
    for n_x in [int(x) for x in a.exhaustive.split(",")]:
        qx = queries[:n_x].contiguous()
        calls, outs = {}, {}
        for n, r in refiners.items():
            ol = torch.empty((n_x, k), dtype=torch.int32, device=dev)
            od = torch.empty((n_x, k), dtype=torch.float32, device=dev)
            outs[n] = (ol, od)
            calls[n] = (lambda r=r, ol=ol, od=od, qx=qx, n_x=n_x: _lib.check(L.vaqhip_refiner_search_device(
                r._h, p(qx), n_x, k, p(ol), p(od), C.c_void_p(st))))
        run_leg({"call": "exhaustive", "queries": n_x, "lane_ops": 3 * n_x * N * D}, calls, outs)
    rf.close(), r8.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
