"""Encoding from byte rows next to encoding from the same rows widened to float32.

    python tools/bench_encode_u8.py --out profiles/encode_u8_1m.json

Workload (tools/bench_encode_multi.py's, byte-valued): 1M x 128 rows of uint8 over the whole range, M = 8 subspaces x 8
bits, a rotation (projected = 0).  Pairs, alternating in one process after a warm-up, codes asserted equal on every
repetition:
  single    vaqhip_encode(X.astype(float32))            against vaqhip_encode_u8(X)              host forms, upload included
  host      vaqhip_multi_encode_set_codes(float rows)   against vaqhip_multi_encode_set_codes_u8 host forms, upload included
  refiner   vaqhip_multi_encode_from_refiner over a float refiner against the same over a byte refiner (rows resident)
The multi forms run over G logical shards of GPU 0: that measures the mechanism, not scaling.  Wall time around the
synchronous call: median, min, max of the repeats; encode_ms / set_codes_ms are the library's own device events
(vaqhip_multi_last_encode_timing, slowest shard).  Nothing is fixed in advance: the file holds what was measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "runs_ms": [round(m, 3) for m in ms]}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--subspaces", type=int, default=8)
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--shards", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_u8_1m.json"))
    a = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import build
    from vaq_amd.index import VaqHipMulti
    rng = np.random.default_rng(23)
    D, M, n = a.dim, a.subspaces, a.rows
    X8 = rng.integers(0, 256, size=(n, D), dtype=np.uint8)
    Xf = X8.astype(np.float32)
    cents = [(rng.normal(size=(1 << a.bits, D // M)) * 60 + 100).astype(np.float32) for _ in range(M)]
    eig = np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32)
    res = dict(tool="tools/bench_encode_u8.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0),
               gpus_used=1, rows=n, dim=D, subspaces=M, bits=a.bits, projected=0, repeats=a.repeats,
               float_row_bytes=n * D * 4, byte_row_bytes=n * D,
               timing="wall ms around the synchronous call; float and byte form alternate in one process after one warm-up "
                      "pair; codes asserted equal on every repetition; multi forms return the codes to the host both ways",
               shards="logical shards of one GPU: the cost of the mechanism, not scaling", pairs={})

    def pair(name, f_float, f_byte, phases=None):
        f_float(), f_byte()  # warm-up
        t = {"float32": [], "uint8": []}
        ph = {"float32": None, "uint8": None}
        for _ in range(a.repeats):
            ms, want = timed(f_float)
            t["float32"].append(ms)
            if phases:
                ph["float32"] = phases()
            ms, got = timed(f_byte)
            t["uint8"].append(ms)
            if phases:
                ph["uint8"] = phases()
            assert np.array_equal(got, want), name
        out = {k: stats(v) for k, v in t.items()}
        if phases:
            for k in ph:
                out[k]["last_phases_ms"] = {x: round(y, 3) for x, y in ph[k].items() if x.endswith("_ms")}
        lo, hi = out["uint8"], out["float32"]
        out["ranges_overlap"] = not (lo["max_ms"] < hi["min_ms"] or hi["max_ms"] < lo["min_ms"])
        out["codes_equal"] = True
        res["pairs"][name] = out
        print(name, json.dumps(out), flush=True)

    v = vaq_amd.VaqHip()
    v.mBitsAlloc, v.mCentroidsPerSubs, v.mEigenVectors = [a.bits] * M, cents, eig

    def one(fn, X):
        fn(X, projected=False)
        return v.mCodebook

    pair("single", lambda: one(v.encode, Xf), lambda: one(v.encode_u8, X8))
    v.close()
    for G in a.shards:
        devices = [0] * G
        m = VaqHipMulti(devices, [a.bits] * M, cents, eig)
        pair(f"host_G{G}", lambda: m.encode(Xf, projected=False, return_codes=True),
             lambda: m.encode_u8(X8, projected=False, return_codes=True), m.last_encode_timing)
        rf, r8 = vaq_amd.VaqMultiRefiner(devices, D), vaq_amd.VaqMultiRefiner(devices, D)
        rf.set_rows(Xf)
        r8.set_rows_u8(X8)
        pair(f"refiner_G{G}", lambda: m.encode_from_refiner(rf, return_codes=True),
             lambda: m.encode_from_refiner(r8, return_codes=True), m.last_encode_timing)
        for x in (m, rf, r8):
            x.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
