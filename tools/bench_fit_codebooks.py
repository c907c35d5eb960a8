"""Fitting the subspace codebooks on the GPU (vaqhip_fit_codebooks_device / _u8_device) at 1M x 128 byte-valued rows.
Writes one JSON file (default profiles/fit_codebooks_1m.json) and prints it.  Per shape -- C2 (8 x 8 bits), C3
({12,10,9,8,8,7,6,4}), FAST (64 x 4 bits) -- the float and the byte form alternate in one process, `--runs` repetitions
each after a warm-up of both, every result asserted bit-equal to the first:

  total_ms        host clock around the call, which synchronises before it returns: median, min, max and every run
  phases_ms       from one more call per form with vaqhip_fit_codebooks_set_timing(1) (one synchronisation per phase):
                  gather + project + seeds, assign, sort + run bounds + ordered sums, update
  iterations      the reference's iter_count per subspace; nan_rows: centres an empty cluster left NaN
  peak_device_bytes  the largest drop of hipMemGetInfo's free bytes seen by a polling thread during a call

No threshold is asserted: nothing about this path's speed was promised.  The rows are resident on the device before
the clock starts (the _device forms); the sample is gathered from them on the device.

    python tools/bench_fit_codebooks.py [--rows 1000000 --runs 5 --out profiles/fit_codebooks_1m.json --commit <id>]
    python tools/bench_fit_codebooks.py --once C2     (one shape, byte form, a warm-up call and a timed one: the run a
                                                       kernel trace is taken of -- every kernel count is two fits')
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

D = 128
SHAPES = {"C2": [8] * 8, "C3": [12, 10, 9, 8, 8, 7, 6, 4], "FAST": [4] * 64}


def make_rows(rows):
    """byte-valued rows with a SIFT-like skew (most values small), as a bvecs file holds them"""
    rng = np.random.default_rng(13517106)
    return np.minimum(rng.gamma(1.2, 22.0, size=(rows, D)), 255.0).astype(np.uint8)


def stats(ms):
    s = sorted(ms)
    med = s[len(s) // 2]
    return {"median_ms": round(med, 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3),
            "spread_pct": round(100.0 * (s[-1] - s[0]) / med, 2), "runs_ms": [round(m, 3) for m in ms]}


class PeakMemory:
    """polls hipMemGetInfo while a call runs: the largest amount in use above what was in use when it started"""

    def __init__(self, torch):
        self.torch = torch
        self.peak = 0

    def __enter__(self):
        self.base = self.torch.cuda.mem_get_info()[0]
        self.stop = False
        self.th = threading.Thread(target=self.poll)
        self.th.start()
        return self

    def poll(self):
        while not self.stop:
            self.peak = max(self.peak, self.base - self.torch.cuda.mem_get_info()[0])
            time.sleep(0.0005)

    def __exit__(self, *a):
        self.stop = True
        self.th.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_codebooks_1m.json"))
    ap.add_argument("--commit", default="", help="recorded as given: the commit this build sits on")
    ap.add_argument("--once", default="", help="C2, C3 or FAST: one byte-form call after a warm-up, nothing written")
    args = ap.parse_args()
    import torch
    from vaq_amd import _lib, build
    L = _lib.load()
    n = args.rows
    X8 = make_rows(n)
    d8 = torch.from_numpy(X8).cuda()
    df = d8.to(torch.float32)
    torch.cuda.synchronize()

    def fit(dx, bits):
        M = len(bits)
        ks = [1 << b for b in bits]
        dc = torch.empty(sum(ks) * (D // M), dtype=torch.float32, device="cuda")
        iters, nan = np.zeros(M, np.int32), np.zeros(M, np.int32)
        fn = L.vaqhip_fit_codebooks_u8_device if dx.dtype == torch.uint8 else L.vaqhip_fit_codebooks_device
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(fn(0, C.c_void_p(dx.data_ptr()), n, D, M, (C.c_int * M)(*bits), None, 25, C.c_void_p(dc.data_ptr()),
                      iters.ctypes.data_as(C.c_void_p), nan.ctypes.data_as(C.c_void_p), None))
        ms = (time.perf_counter() - t0) * 1e3
        return ms, dc.cpu().numpy().view(np.uint32), iters, nan

    def phases(dx, bits):
        L.vaqhip_fit_codebooks_set_timing(1)
        with PeakMemory(torch) as pm:
            fit(dx, bits)
        L.vaqhip_fit_codebooks_set_timing(0)
        t = _lib.FitCodebooksTiming()
        _lib.check(L.vaqhip_last_fit_codebooks_timing(C.byref(t)))
        return {"gather_project_seed": round(t.gather_ms, 3), "assign": round(t.assign_ms, 3),
                "sort_accumulate": round(t.accumulate_ms, 3), "update": round(t.update_ms, 3),
                "total_with_phase_synchronisations": round(t.total_ms, 3), "sample_rows": int(t.sample_rows),
                "largest_iteration_count": int(t.iterations)}, int(pm.peak)

    if args.once:
        fit(d8, SHAPES[args.once])  # code objects, rocprim's kernels: the trace holds this shape twice, nothing else
        ms, _, iters, _ = fit(d8, SHAPES[args.once])
        print(json.dumps({"shape": args.once, "total_ms": round(ms, 3), "iterations": iters.tolist()}), flush=True)
        return

    out = {"workload": f"KMeans::staticFitSampling per subspace, max_iter 25: {n} x {D} byte-valued rows resident on the device, "
                       "no rotation; float and byte form alternating",
           "gpu": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "commit": args.commit, "shapes": {}}
    for name, bits in SHAPES.items():
        _, want, iters, nan = fit(df, bits)  # warm-up of both forms, and the yardstick
        fit(d8, bits)
        t_f, t_8 = [], []
        for _ in range(args.runs):
            for dx, acc in ((df, t_f), (d8, t_8)):
                ms, got, it, nn = fit(dx, bits)
                assert np.array_equal(got, want) and np.array_equal(it, iters) and np.array_equal(nn, nan), name
                acc.append(ms)
        ph_f, peak_f = phases(df, bits)
        ph_8, peak_8 = phases(d8, bits)
        out["shapes"][name] = {"bits": bits, "iterations": iters.tolist(), "nan_rows": nan.tolist(),
                               "results_bit_equal_on_every_run": True,
                               "float_rows": dict(stats(t_f), phases_ms=ph_f, peak_device_bytes=peak_f),
                               "byte_rows": dict(stats(t_8), phases_ms=ph_8, peak_device_bytes=peak_8)}
        print(name, json.dumps(out["shapes"][name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
