"""The sharded build of a queryLUT index (vaqhip_multi_lut_fit_quantiles, vaqhip_multi_encode_lut_set_codes) against
the single-device calls on the workload of tools/bench_lut_fit.py: 1M x 128 projected rows, the 233-bit allocation.
On a machine with one GPU the shards are logical shards of that GPU ([0] * G): their chains share one device and cannot
overlap, so this measures the scheme's overhead, not a speed-up; distinct GPUs are not measured by it.

  fit     vaqhip_lut_fit_quantiles (host form, one device) alternating with the sharded fit at G = 1, 2, 4, 8 in one
          process: wall ms of each call (median, min, max over the repeats), the sharded fit's per-phase device times,
          and the assertion that every result is bit-equal to the single fit's
  encode  vaqhip_encode_lut + vaqhip_multi_set_codes_u16 alternating with vaqhip_multi_encode_lut_set_codes in the same
          way, codes asserted equal

    python tools/bench_lut_fit_multi.py [--rows 1000000 --runs 5 --out profiles/lut_fit_multi_1m.json --commit <id>]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_lut_fit import BITS, D, make_rows, stats  # noqa: E402

GS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lut_fit_multi_1m.json"))
    ap.add_argument("--commit", default="", help="recorded as given: the commit this build sits on")
    args = ap.parse_args()
    runs = max(args.runs, 5)
    import torch
    import vaq_amd
    from vaq_amd import _lib, build
    from vaq_amd.index import VaqHipMulti
    L = _lib.load()
    n = args.rows
    X = make_rows(n)
    bits = (C.c_int * D)(*BITS)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def single_fit(rows):
        cent, q = np.empty((D, 256), np.float32), np.empty((D, 257), np.float32)
        t0 = time.perf_counter()
        _lib.check(L.vaqhip_lut_fit_quantiles(args.device, p(X), rows, D, bits, None, p(cent), p(q)))
        return (time.perf_counter() - t0) * 1e3, cent, q

    def multi_fit(G, rows):
        t0 = time.perf_counter()
        cent, q = vaq_amd.lut_fit_quantiles_multi([args.device] * G, X[:rows], BITS)
        return (time.perf_counter() - t0) * 1e3, cent, q, vaq_amd.last_lut_fit_multi_timing()

    single_fit(min(n, 4096))  # warm-up: code objects, rocprim's kernels
    for G in GS:
        multi_fit(G, min(n, 4096))
    _, cent0, q0 = single_fit(n)
    t_single, t_multi, phases = [], {G: [] for G in GS}, {}
    for _ in range(runs):
        t_single.append(single_fit(n)[0])
        for G in GS:
            ms, cent, q, tm = multi_fit(G, n)
            assert np.array_equal(cent.view(np.uint32), cent0.view(np.uint32)), f"G={G}: centres differ"
            assert np.array_equal(q.view(np.uint32), q0.view(np.uint32)), f"G={G}: quantiles differ"
            t_multi[G].append(ms)
            phases[G] = {k: round(v, 3) for k, v in tm.items() if k.endswith("_ms")}
    out = {"workload": f"binaryEncodingLUT from the bit allocation on: {n} x {D} projected rows on the host, "
                       f"{sum(BITS)} code bits; wall time of the host-form calls, upload included",
           "gpu": torch.cuda.get_device_name(0), "gpus_used": 1, "shards": "logical shards of one GPU",
           "source_hash": build.source_hash(), "commit": args.commit,
           "fit": {"vaqhip_lut_fit_quantiles": stats(t_single),
                   "vaqhip_multi_lut_fit_quantiles": {str(G): dict(stats(t_multi[G]), last_phases_ms=phases[G]) for G in GS},
                   "bit_equal": True}}

    # ---- encode: single encoder + set_codes_u16 against the encode across the shards ----
    cents = [np.ascontiguousarray(cent0[d, :1 << b].reshape(-1, 1)) for d, b in enumerate(BITS)]
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(BITS)
    v.mCentroidsPerSubs = cents
    v.mQuantiles = q0
    v._ensure_quantiles()
    codes = np.empty((n, D), np.uint16)
    enc = {}
    for G in GS:
        a = VaqHipMulti([args.device] * G, BITS, cents, sequential_sum=True)
        b = VaqHipMulti([args.device] * G, BITS, cents, sequential_sum=True)
        a.set_lut_quantiles(q0)
        t_old, t_new = [], []
        for i in range(runs + 1):
            t0 = time.perf_counter()
            _lib.check(L.vaqhip_encode_lut(v._h, p(X), n, 1, p(codes)))
            b.set_codes(codes)
            t1 = time.perf_counter()
            got = a.encode_lut(X, projected=True, return_codes=(i == 0))
            t2 = time.perf_counter()
            if i == 0:  # (the warm-up pass carries the check)
                assert np.array_equal(got, codes), f"G={G}: codes differ"
                continue
            t_old.append((t1 - t0) * 1e3)
            t_new.append((t2 - t1) * 1e3)
        et = a.last_encode_timing()
        enc[str(G)] = {"encode_lut_then_set_codes_u16": stats(t_old), "multi_encode_lut_set_codes": stats(t_new),
                       "last_phases_ms": {k: round(x, 3) for k, x in et.items() if k.endswith("_ms")}}
        a.close(), b.close()
    out["encode"] = dict(enc, codes_equal=True, note="the old route returns the codes to the host and uploads them again; "
                                                     "the new route is timed without codes_out")
    v.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
