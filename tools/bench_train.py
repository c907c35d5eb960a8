"""Training from raw rows (vaqhip_refiner_train_rotation) at 1M x 128 byte-valued rows resident in a refiner, the float
and the byte form alternating in one process, `--runs` repetitions each after a warm-up of both, every result asserted
equal to the first.  Writes one JSON file (default profiles/train_1m.json) and prints it:

  total_ms        host clock around the call: median, min, max and every run
  phases_ms       from the call's own timing struct: second moment, solver (of which the host finish), plan + allocation;
                  sweeps; sample_rows (1000 * D = 128 000 of the 1M rows)
  moment_tflops   the multiply-adds the moment kernel executes (the upper triangle of 32 x 32 blocks) over moment_ms,
                  next to the MI355X's vector fp64 peak
  yardstick       what harness.pca_eigenvectors does today on the same rows in the same process: a torch double matmul
                  on the device plus eigh on the CPU.  Only a yardstick: it samples other rows and allocates no bits.
  allocate_ms     vaqhip_allocate_bits alone at the two headline shapes (host only)
  d960            where memory allows, one D = 960, n = 100 000 float case: what the launch-per-step Jacobi and its
                  host finish cost at GIST width

No threshold is asserted.  Not run: distinct GPUs, anything near 1B rows (the sample bounds the work there; unmeasured).

    python tools/bench_train.py [--rows 1000000 --runs 5 --out profiles/train_1m.json --commit <id> --no-d960]
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

FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X data sheet: vector FP64
D, M, BUDGET, MIN_BITS, MAX_BITS = 128, 16, 128, 1, 12


def make_rows(rows, dims):
    """byte-valued rows with a SIFT-like skew, correlated along the row so that the spectrum decays"""
    rng = np.random.default_rng(13517106)
    base = rng.gamma(1.2, 22.0, size=(rows, dims)).astype(np.float32)
    base[:, 1:] = 0.6 * base[:, 1:] + 0.4 * base[:, :-1]
    return np.minimum(base, 255.0).astype(np.uint8)


def stats(ms):
    s = sorted(ms)
    med = s[len(s) // 2]
    return {"median_ms": round(med, 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3),
            "spread_pct": round(100.0 * (s[-1] - s[0]) / med, 2), "runs_ms": [round(m, 3) for m in ms]}


def moment_flops(sample, dims):
    nb = (dims + 31) // 32
    return 2.0 * sample * (nb * (nb + 1) // 2) * 32 * 32


def timed(refiner, args):
    import vaq_amd
    t0 = time.perf_counter()
    out = refiner.train_rotation(*args)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, out, vaq_amd.last_train_timing()


def phases(t):
    return {"moment_ms": round(t["moment_ms"], 3), "eigen_ms": round(t["eigen_ms"], 3),
            "of_which_host_finish_ms": round(t["finish_ms"], 3), "plan_ms": round(t["plan_ms"], 3), "sweeps": t["sweeps"],
            "sample_rows": t["sample_rows"],
            "moment_tflops": round(moment_flops(t["sample_rows"], t["dims"]) / (t["moment_ms"] * 1e-3) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_1m.json"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--no-d960", action="store_true")
    a = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import _lib, build, harness
    X8 = make_rows(a.rows, D)
    args = (M, BUDGET, MIN_BITS, MAX_BITS)
    forms = {}
    for name, rows in (("float", X8.astype(np.float32)), ("u8", X8)):
        r = vaq_amd.VaqRefiner(D)
        (r.set_rows_u8 if name == "u8" else r.set_rows)(rows)
        forms[name] = r
    first = None
    for r in forms.values():  # warm-up of both
        _, first, _ = timed(r, args)
    runs = {k: [] for k in forms}
    last = {}
    for _ in range(a.runs):
        for name, r in forms.items():
            ms, out, t = timed(r, args)
            assert np.array_equal(out[0], first[0]) and out[2] == first[2], name
            runs[name].append(ms)
            last[name] = t
    res = {"workload": f"{a.rows} x {D} byte-valued rows resident in a refiner; M={M}, budget {BUDGET}, bits {MIN_BITS}..{MAX_BITS}",
           "source_hash": build.source_hash(), "commit": a.commit, "bits": first[2],
           "fp64_vector_peak_tflops": FP64_VECTOR_PEAK_TFLOPS,
           "forms": {k: {"total": stats(v), "phases_of_last_run": phases(last[k])} for k, v in runs.items()}}
    # the yardstick: what the harness does today, same rows, same process
    d_X = torch.from_numpy(X8.astype(np.float32)).cuda()
    harness.pca_eigenvectors(d_X)
    ys = []
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        harness.pca_eigenvectors(d_X)
        torch.cuda.synchronize()
        ys.append((time.perf_counter() - t0) * 1e3)
    res["yardstick_harness_pca_eigenvectors"] = stats(ys)
    del d_X
    for r in forms.values():
        r.close()
    # the allocation alone (host)
    L = _lib.load()
    rng = np.random.default_rng(7)
    res["allocate_ms"] = {}
    for m, b, lo, hi in ((16, 128, 1, 12), (32, 256, 2, 13)):
        c = np.sort((rng.random(m) ** 3 + 1e-3).astype(np.float32))[::-1].copy()
        c /= c.sum()
        lb = np.full(m, lo, np.int32)
        k = np.array([max(int(2.0 ** np.floor(np.log2(c[i] / c[i + 1]))), 0) for i in range(m - 1)] + [0], np.int32)
        bits, obj = np.zeros(m, np.int32), C.c_double(0)
        t0 = time.perf_counter()
        rc = L.vaqhip_allocate_bits(c.ctypes.data_as(C.c_void_p), m, lb.ctypes.data_as(C.c_void_p), hi,
                                    k.ctypes.data_as(C.c_void_p), b, bits.ctypes.data_as(C.c_void_p), C.byref(obj))
        res["allocate_ms"][f"M{m}_B{b}_bits{lo}..{hi}"] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "rc": rc,
                                                           "bits": bits.tolist()}
    if not a.no_d960:
        try:
            Xg = make_rows(100_000, 960).astype(np.float32)
            r = vaq_amd.VaqRefiner(960)
            r.set_rows(Xg)
            ms, out, t = timed(r, (16, 128, 1, 12))
            r.close()
            res["d960"] = {"workload": "100000 x 960 float rows, M=16, budget 128, bits 1..12, one run, no warm-up",
                           "total_ms": round(ms, 3), "phases": phases(t), "bits": out[2]}
        except vaq_amd.VaqHipError as e:  # (memory)
            res["d960"] = {"not_run": str(e)}
    res["not_run"] = "distinct GPUs; anything near 1B rows (the sample bounds the work there, but nobody has measured it)"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
