"""Building a multi-device index from raw rows: the encode across the shards next to the route it replaces.

    python tools/bench_encode_multi.py --out profiles/encode_multi_1m.json

Workload: 1M x 128 raw float rows, M = 8 subspaces x 8 bits, a rotation (projected = 0).  Three routes, alternating in
one process after a warm-up, each leaving the index in the same state:
  parent    vaqhip_encode of all rows on shard 0 into host memory, then vaqhip_multi_set_codes_u16 (every code crosses
            to the host and back; the rows go through one GPU)
  host      vaqhip_multi_encode_set_codes: every shard uploads and encodes its slice and keeps the codes
  refiner   vaqhip_multi_encode_from_refiner: the rows are resident in a multi refiner (uploaded once, not timed here;
            `refiner_upload_ms` says what that cost), every shard encodes them in place
G = 1, 2, 4, 8 shards over distinct GPUs where the machine has that many, logical shards on GPU 0 otherwise -- the file
says which; on logical shards the figures are the cost of the mechanism, not scaling.  The calls are synchronous: wall
time around the call, median / min / max of the repeats; encode_ms and set_codes_ms are the call's own device events
(slowest shard).  Nothing is fixed in advance: the file holds what was measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--subspaces", type=int, default=8)
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--shards", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--key", default="", help="store the runs under this key of an existing --out file (e.g. distinct_gpus)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_multi_1m.json"))
    a = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import _lib, build
    from vaq_amd.index import VaqHipMulti
    L = _lib.load()
    n_gpus = torch.cuda.device_count()
    rng = np.random.default_rng(23)
    D, M = a.dim, a.subspaces
    X = rng.standard_normal(size=(a.rows, D), dtype=np.float32) * np.float32(30)
    cents = [(rng.normal(size=(1 << a.bits, D // M)) * 30).astype(np.float32) for _ in range(M)]
    eig = np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32)
    codes = np.empty((a.rows, M), np.uint16)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    res = dict(tool="tools/bench_encode_multi.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0),
               gpus=n_gpus, rows=a.rows, dim=D, subspaces=M, bits=a.bits, projected=0, repeats=a.repeats,
               timing="wall time around the synchronous call, median of %d, the three routes alternating in one process "
                      "after one warm-up round; encode_ms / set_codes_ms: device events of the slowest shard" % a.repeats,
               runs=[])
    for G in a.shards:
        distinct = n_gpus >= G
        devices = list(range(G)) if distinct else [0] * G
        m = VaqHipMulti(devices, [a.bits] * M, cents, eig)
        r = vaq_amd.VaqMultiRefiner(devices, D)
        upload_ms = wall_ms(lambda: r.set_rows(X))

        def parent():
            _lib.check(L.vaqhip_encode(m.shard(0), ptr(X), a.rows, 0, ptr(codes)))
            m.set_codes(codes)

        routes = dict(parent=parent, host=lambda: m.encode(X, projected=False), refiner=lambda: m.encode_from_refiner(r))
        parent()
        assert np.array_equal(m.encode(X, projected=False, return_codes=True), codes)
        assert np.array_equal(m.encode_from_refiner(r, return_codes=True), codes)
        t = {k: [] for k in routes}
        ph = {k: [] for k in ("host", "refiner")}
        for _ in range(a.repeats):
            for k, fn in routes.items():
                t[k].append(wall_ms(fn))
                if k in ph:
                    e = m.last_encode_timing()
                    ph[k].append((e["encode_ms"], e["set_codes_ms"]))
        med = lambda v: round(statistics.median(v), 3)
        run = dict(shards=G, placement="one GPU" if G == 1 else "distinct GPUs" if distinct else "logical shards on GPU 0",
                   refiner_upload_ms=round(upload_ms, 3), row_bytes=a.rows * D * 4, code_bytes=a.rows * M * 2)
        for k in routes:
            run[k + "_ms"] = med(t[k])
            run[k + "_min_ms"] = round(min(t[k]), 3)
            run[k + "_max_ms"] = round(max(t[k]), 3)
        for k in ph:
            run[k + "_encode_ms"] = med([p[0] for p in ph[k]])
            run[k + "_set_codes_ms"] = med([p[1] for p in ph[k]])
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        m.close()
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.key and os.path.exists(a.out):
        whole = json.load(open(a.out))
        whole[a.key] = res
        res = whole
    elif n_gpus < max(a.shards):
        res["distinct_gpus"] = "not measured"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
