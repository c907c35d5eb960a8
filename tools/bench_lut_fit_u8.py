"""The quantile fit from byte rows next to the fit from the same rows widened to float32.

    python tools/bench_lut_fit_u8.py --out profiles/lut_fit_u8_1m.json

Workload (tools/bench_lut_fit_multi.py's, byte-valued): 1M x 128 rows of uint8 over the whole range, the 233-bit
allocation, no rotation.  Pairs, alternating in one process after a warm-up, results asserted bit-equal on every
repetition:
  single    vaqhip_lut_fit_quantiles(X.astype(float32))       against vaqhip_lut_fit_quantiles_u8(X)
  host      vaqhip_multi_lut_fit_quantiles(float rows)        against vaqhip_multi_lut_fit_quantiles_u8   (upload included)
  refiner   vaqhip_multi_refiner_lut_fit_quantiles over a float refiner against the same over a byte refiner
The sharded forms run over G logical shards of GPU 0: that measures the mechanism, not scaling.  Wall ms around the
synchronous call (median, min, max) and the library's phase times of the last call (vaqhip_last_lut_fit_timing,
vaqhip_multi_last_lut_fit_timing).  Nothing is fixed in advance: the file holds what was measured."""
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

from bench_lut_fit import BITS, D, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shards", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lut_fit_u8_1m.json"))
    a = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import _lib, build
    L = _lib.load()
    n = a.rows
    X8 = np.random.default_rng(13517106).integers(0, 256, size=(n, D), dtype=np.uint8)
    Xf = X8.astype(np.float32)
    bits = (C.c_int * D)(*BITS)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _lib.check(L.vaqhip_lut_fit_set_timing(1))

    def single(fn, X):
        cent, q = np.empty((D, 256), np.float32), np.empty((D, 257), np.float32)
        _lib.check(fn(0, p(X), n, D, bits, None, p(cent), p(q)))
        return cent, q

    def single_phases():
        t = _lib.LutFitTiming()
        _lib.check(L.vaqhip_last_lut_fit_timing(C.byref(t)))
        return {f: getattr(t, f) for f, _ in t._fields_}

    out = {"tool": "tools/bench_lut_fit_u8.py", "source_hash": build.source_hash(), "gpu": torch.cuda.get_device_name(0),
           "gpus_used": 1, "shards": "logical shards of one GPU: the cost of the mechanism, not scaling",
           "workload": f"{n} x {D} byte-valued rows, {sum(BITS)} code bits, no rotation; wall ms of the synchronous call, "
                       "float and byte form alternating, results asserted bit-equal on every repetition",
           "float_row_bytes": n * D * 4, "byte_row_bytes": n * D, "pairs": {}}

    def pair(name, f_float, f_byte, phases):
        f_float(), f_byte()  # warm-up
        t = {"float32": [], "uint8": []}
        ph = {}
        for _ in range(max(a.runs, 5)):
            t0 = time.perf_counter()
            wc, wq = f_float()
            t["float32"].append((time.perf_counter() - t0) * 1e3)
            ph["float32"] = phases()
            t0 = time.perf_counter()
            gc, gq = f_byte()
            t["uint8"].append((time.perf_counter() - t0) * 1e3)
            ph["uint8"] = phases()
            assert np.array_equal(gc.view(np.uint32), wc.view(np.uint32)) and np.array_equal(gq.view(np.uint32), wq.view(np.uint32)), name
        r = {k: dict(stats(v), last_phases_ms={x: round(y, 3) for x, y in ph[k].items() if x.endswith("_ms")}) for k, v in t.items()}
        lo, hi = r["uint8"], r["float32"]
        r["ranges_overlap"] = not (lo["max_ms"] < hi["min_ms"] or hi["max_ms"] < lo["min_ms"])
        r["bit_equal"] = True
        out["pairs"][name] = r
        print(name, json.dumps(r), flush=True)

    pair("single", lambda: single(L.vaqhip_lut_fit_quantiles, Xf), lambda: single(L.vaqhip_lut_fit_quantiles_u8, X8), single_phases)
    for G in a.shards:
        devices = [0] * G
        pair(f"host_G{G}", lambda: vaq_amd.lut_fit_quantiles_multi(devices, Xf, BITS),
             lambda: vaq_amd.lut_fit_quantiles_multi_u8(devices, X8, BITS), vaq_amd.last_lut_fit_multi_timing)
        rf, r8 = vaq_amd.VaqMultiRefiner(devices, D), vaq_amd.VaqMultiRefiner(devices, D)
        rf.set_rows(Xf)
        r8.set_rows_u8(X8)
        pair(f"refiner_G{G}", lambda: rf.fit_quantiles(BITS), lambda: r8.fit_quantiles(BITS), vaq_amd.last_lut_fit_multi_timing)
        rf.close(), r8.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
