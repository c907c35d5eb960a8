"""Building a queryLUT index on the GPU (vaqhip_lut_fit_quantiles_device, vaqhip_encode_lut_device) at 1M x 128
projected rows, bits per dimension from the C3-like spread cut to at most 8 (233 code bits: an index packs at
most 256).  Writes one JSON file (default profiles/lut_fit_1m.json) and prints it:

  fit     total ms of a call (every run listed) and, from one more call with vaqhip_lut_fit_set_timing(1), the
          device time per phase; next to them the same rows through vaq_lutfit.h on ONE CPU thread
          (tools/lut_fit_cpu.cpp) -- the reference's shape of the work; recorded, no ratio promised -- and whether
          the two results are bit-equal
  encode  vaqhip_encode_lut_device against vaqhip_encode_device (untouched by this feature, so the code of the
          commit before it) on the same index and rows, alternating in one process: median, min and the
          run-to-run spread of each

    python tools/bench_lut_fit.py [--rows 1000000 --runs 5 --out profiles/lut_fit_1m.json --commit <id>]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

D = 128
BITS = [8, 8, 8, 8, 8, 7, 6, 4] + [3] * 16 + [2] * 24 + [1] * 80  # harness.C3_BITS cut to 8, then a tail


def make_rows(rows):
    rng = np.random.default_rng(13517106)
    scale = (40.0 / np.sqrt(1.0 + np.arange(D))).astype(np.float32)  # a PCA spectrum: decaying
    return (rng.standard_normal(size=(rows, D), dtype=np.float32) * scale).astype(np.float32)


def cpu_lib(tmp):
    so = os.path.join(tmp, "lut_fit_cpu.so")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "vaq_amd", "csrc"),
                           os.path.join(ROOT, "tools", "lut_fit_cpu.cpp"), "-o", so])
    return C.CDLL(so)


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "spread_pct": round(100.0 * (ms[-1] - ms[0]) / med, 2), "runs_ms": [round(m, 3) for m in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lut_fit_1m.json"))
    ap.add_argument("--commit", default="", help="recorded as given: the commit this build sits on")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import _lib, build
    L = _lib.load()
    n = args.rows
    X = make_rows(n)
    bits = (C.c_int * D)(*BITS)
    dx = torch.from_numpy(X).cuda()
    dc = torch.empty((D, 256), dtype=torch.float32, device="cuda")
    dq = torch.empty((D, 257), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fit(rows):
        _lib.check(L.vaqhip_lut_fit_quantiles_device(0, C.c_void_p(dx.data_ptr()), rows, D, bits, None,
                                                     C.c_void_p(dc.data_ptr()), C.c_void_p(dq.data_ptr()), st))
        t = _lib.LutFitTiming()
        _lib.check(L.vaqhip_last_lut_fit_timing(C.byref(t)))
        return t

    fit(min(n, 4096))  # warm-up: code objects, rocprim's kernels
    fit(n)
    totals = [fit(n).total_ms for _ in range(args.runs)]
    L.vaqhip_lut_fit_set_timing(1)
    tp = fit(n)
    L.vaqhip_lut_fit_set_timing(0)
    cent = np.ascontiguousarray(dc.cpu().numpy())
    Q = np.ascontiguousarray(dq.cpu().numpy())
    out = {"workload": f"binaryEncodingLUT from the bit allocation on: {n} x {D} projected rows, bits {BITS[:8]} + "
                       f"16x3 + 24x2 + 80x1 ({sum(BITS)} code bits)",
           "gpu": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "commit": args.commit,
           "fit": dict(stats(totals), phases_ms={"extract": round(tp.extract_ms, 3), "sort": round(tp.sort_ms, 3),
                                                 "quantiles": round(tp.quantile_ms, 3), "means": round(tp.means_ms, 3)},
                       total_ms_with_phase_events=round(tp.total_ms, 3))}

    # ---- encode: the new encoder against vaqhip_encode_device, same index, same rows, alternating ----
    v = vaq_amd.VaqHip(sequential_sum=True)
    v.mBitsAlloc = list(BITS)
    v.mCentroidsPerSubs = [np.ascontiguousarray(cent[d, :1 << b].reshape(-1, 1)) for d, b in enumerate(BITS)]
    v.mQuantiles = Q
    v._ensure_quantiles()
    codes_lut = torch.empty((n, D), dtype=torch.int16, device="cuda")
    codes_old = torch.empty((n, D), dtype=torch.int16, device="cuda")

    def timed(fn, dst):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(fn(v._h, C.c_void_p(dx.data_ptr()), n, 1, C.c_void_p(dst.data_ptr()), st))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):
        timed(L.vaqhip_encode_lut_device, codes_lut)
        timed(L.vaqhip_encode_device, codes_old)
    t_lut, t_old = [], []
    for _ in range(max(args.runs, 3) * 2):
        t_lut.append(timed(L.vaqhip_encode_lut_device, codes_lut))
        t_old.append(timed(L.vaqhip_encode_device, codes_old))
    differ = int((codes_lut != codes_old).sum().item())
    out["encode"] = {"encode_lut_device": stats(t_lut), "vaqhip_encode_device": stats(t_old),
                     "bytes_read_and_written": n * D * 6,
                     "codes_differing_from_first_argmin": differ, "codes": n * D}

    if not args.no_cpu:
        with tempfile.TemporaryDirectory() as tmp:
            cl = cpu_lib(tmp)
            ccent = np.empty((D, 256), np.float32)
            cq = np.empty((D, 257), np.float32)
            ccodes = np.empty((n, D), np.uint16)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            cl.lut_fit_cpu.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
            cl.lut_encode_cpu.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
            t0 = time.perf_counter()
            cl.lut_fit_cpu(p(X), n, D, bits, p(ccent), p(cq))
            t1 = time.perf_counter()
            cl.lut_encode_cpu(p(X), n, D, bits, p(ccent), p(cq), p(ccodes))
            t2 = time.perf_counter()
        out["cpu_one_thread"] = {
            "fit_ms": round((t1 - t0) * 1e3, 1), "encode_ms": round((t2 - t1) * 1e3, 1),
            "fit_bit_equal_to_gpu": bool(np.array_equal(ccent.view(np.uint32), cent.view(np.uint32))
                                         and np.array_equal(cq.view(np.uint32), Q.view(np.uint32))),
            "codes_equal_to_gpu": bool(np.array_equal(ccodes, codes_lut.cpu().numpy().view(np.uint16)))}
    v.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
