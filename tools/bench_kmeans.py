"""The k-means of VAQ::clusterTI(true) (vaqhip_index_cluster_ti_kmeans) at the paper's TI shape: T = 1000
centres over 1M rows of 8 x 8-bit codes (D = 128, so 16 dims per subspace), seg = 2 and 4 (centres of 32 and
64 dims), 256 * T = 256000 sampled rows, max_iter = 50.  Prints one JSON line: per seg the total time of one
call, the iterations it ran, and -- from a second call with option "timing" = 1, which ends every phase with a
stream synchronisation -- the time per iteration split into assign / accumulate (sort + ordered sums) / update.
Codes are uniform random and the codebooks gaussian with a decaying scale, from a fixed seed.

    python tools/bench_kmeans.py [--rows 1000000 --clusters 1000 --segs 2 4 --max-iter 50 --runs 1]
    python tools/bench_kmeans.py --devices 0,0,0,0   # the multi-device call (vaqhip_multi_cluster_ti_kmeans) on the
        # same inputs, the rows sharded over these devices (a device named twice: logical shards on it)
    python tools/bench_kmeans.py --dump-inputs DIR   # also writes the inputs of every seg (int32 N, seg, L,
        # centroids, T, max_iter; codes N x seg uint16; seg codebooks) to time another implementation on them
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

D, M, BITS = 128, 8, 8


def make_inputs(rows):
    rng = np.random.default_rng(13517106)
    L = D // M
    cents = [(rng.normal(size=(1 << BITS, L)) * 30.0 / (1 + s)).astype(np.float32) for s in range(M)]
    codes = rng.integers(0, 1 << BITS, size=(rows, M), dtype=np.int64).astype(np.uint16)
    return codes, cents


def run(v, T, seg, max_iter, timing):
    """One call on a VaqHip or a VaqHipMulti: (wall ms, iterations, NaN centres, the library's timing)."""
    from vaq_amd import _lib
    L = _lib.load()
    multi = not hasattr(v, "mCodebook")
    v.set_option("timing", 1 if timing else 0)
    iters = C.c_int(0)
    nan_rows = C.c_int(0)
    t = _lib.KmeansTiming()
    t0 = time.perf_counter()
    if multi:
        _lib.check_multi(L.vaqhip_multi_cluster_ti_kmeans(v._h, T, seg, max_iter, None, C.byref(iters), C.byref(nan_rows)))
        wall = (time.perf_counter() - t0) * 1e3
        _lib.check_multi(L.vaqhip_multi_last_kmeans_timing(v._h, C.byref(t)))
    else:
        _lib.check(L.vaqhip_index_cluster_ti_kmeans(v._h, T, seg, max_iter, None, C.byref(iters), C.byref(nan_rows)))
        wall = (time.perf_counter() - t0) * 1e3
        _lib.check(L.vaqhip_last_kmeans_timing(v._h, C.byref(t)))
    return wall, iters.value, nan_rows.value, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--segs", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--dump-inputs", default=None)
    ap.add_argument("--devices", default=None, help="comma-separated device list: time the multi-device call")
    ap.add_argument("--runs", type=int, default=1, help="untimed-phase calls per seg; every total is reported")
    args = ap.parse_args()
    import vaq_amd

    codes, cents = make_inputs(args.rows)
    T = args.clusters
    if args.dump_inputs:
        os.makedirs(args.dump_inputs, exist_ok=True)
        for seg in args.segs:
            with open(os.path.join(args.dump_inputs, f"kmeans_seg{seg}.bin"), "wb") as f:
                f.write(np.array([args.rows, seg, D // M, 1 << BITS, T, args.max_iter], np.int32).tobytes())
                f.write(np.ascontiguousarray(codes[:, :seg]).tobytes())
                for s in range(seg):
                    f.write(cents[s].tobytes())
    if args.devices:
        devices = [int(d) for d in args.devices.split(",")]
        from vaq_amd.index import VaqHipMulti
        v = VaqHipMulti(devices, [BITS] * M, cents)
        v.set_codes(codes)
    else:
        v = vaq_amd.VaqHip(device=0)
        v.mBitsAlloc = [BITS] * M
        v.mCentroidsPerSubs = cents
        v.mCodebook = codes
        v._ensure_codes()
    out = {"workload": f"k-means of clusterTI: T={T}, {args.rows} rows x {M} x {BITS}-bit, D={D}, max_iter={args.max_iter}"}
    if args.devices:
        out["devices"] = devices
    run(v, min(T, 16), args.segs[0], 2, False)  # warm-up: module load, allocations
    for seg in args.segs:
        totals = []
        for _ in range(max(args.runs, 1)):
            wall, iters, nan_rows, t = run(v, T, seg, args.max_iter, False)
            totals.append(round(t.total_ms, 2))
        _, iters2, _, tp = run(v, T, seg, args.max_iter, True)
        assert iters2 == iters
        out[f"seg{seg}"] = {
            "dims": t.dims, "sampled_rows": t.rows, "iterations": iters, "nan_centres": nan_rows,
            "call_ms": round(wall, 2),                       # the whole call: k-means + regrouping the rows
            "kmeans_ms": round(t.total_ms, 2),               # sample, gather, decode, iterations (the last run's)
            "kmeans_ms_runs": totals,
            "assign_ms_per_iter": round(tp.assign_ms / iters, 4),
            "accumulate_ms_per_iter": round(tp.accumulate_ms / iters, 4),
            "update_ms_per_iter": round(tp.update_ms / iters, 4),
            "kmeans_ms_with_phase_syncs": round(tp.total_ms, 2),
        }
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == "__main__":
    main()
