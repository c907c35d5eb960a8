"""learnQuantization: the host form next to the device forms, on the same rows.

    python tools/bench_learn_quantization.py --out profiles/learn_quant_1m.json

Workload: 1M x 128 byte-valued rows, 64 x 4-bit codes, a rotation, ratio 0.1 (100 000 sampled rows, 1.6M table values
per column).  In one process, after a warm-up, five repetitions of: the parent vaqhip_learn_quantization over the rows
as float32, then the _u8 form over the host bytes, the _device form over the floats on the device, and the refiner form
over a byte and over a float refiner.  offsets and scale are asserted bit-equal to the parent's on every repetition.
Wall ms around the synchronous call (median, min, max) and the phase times of vaqhip_last_learn_timing for the last
repetition.  Peak device bytes: one more, untimed call of every form while a thread samples hipMemGetInfo
(torch.cuda.mem_get_info) -- the most by which the free memory fell below its level before the call; the rows resident
beforehand are not in it.
Every GPU step runs under a time limit of its own (--step-limit seconds, the set-up under --setup-limit): a step that
overruns ends the process with status 124 and nothing more is started on the GPU.
Nothing is fixed in advance: the file holds what was measured."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from bench_lut_fit import stats  # noqa: E402


@contextlib.contextmanager
def step_limit(seconds, what):
    """one GPU step's own time limit: an overrun ends the process, as `timeout` would (status 124)"""
    def overrun():
        sys.stderr.write(f"{what}: over its limit of {seconds} s\n")
        sys.stderr.flush()
        os._exit(124)
    t = threading.Timer(seconds, overrun)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def peak_bytes_during(torch, call):
    """bytes by which the device's free memory fell at most while call() ran (hipMemGetInfo, sampled by a thread)"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    low = [free0]
    stop = threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.0002)
    th = threading.Thread(target=sample, daemon=True)
    th.start()
    try:
        call()
    finally:
        stop.set()
        th.join()
    return int(free0 - low[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-limit", type=float, default=30.0)
    ap.add_argument("--setup-limit", type=float, default=120.0)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ratio", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_quant_1m.json"))
    a = ap.parse_args()
    import torch
    import vaq_amd
    from vaq_amd import _lib, build
    from helpers import make_case
    L = _lib.load()
    n, D, M = a.rows, 128, 64
    c = make_case(13, D, [4] * M, 16, 4)
    setup = step_limit(a.setup_limit, "set-up")
    setup.__enter__()
    v = vaq_amd.VaqHipFast(device=0)
    v.parseMethodString(f"VAQ{4 * M}m{M}min1max4var1,FAST")
    v.mBitsAlloc, v.mCentroidsPerSubs, v.mEigenVectors, v.mCodebook = c["bits"], c["cents"], c["eig"], c["codes"]
    v._ensure_codes()
    h = v._h
    X8 = np.random.default_rng(13517106).integers(0, 256, size=(n, D), dtype=np.uint8)
    Xf = X8.astype(np.float32)
    d_f = torch.from_numpy(Xf).cuda()
    d_8 = torch.from_numpy(X8).cuda()
    r8, rf = vaq_amd.VaqRefiner(D, device=0), vaq_amd.VaqRefiner(D, device=0)
    r8.set_rows_u8(X8)
    rf.set_rows(Xf)
    torch.cuda.synchronize()
    setup.__exit__(None, None, None)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    ratio = C.c_float(a.ratio)

    def call(fn, *args):
        off, sc = np.empty(M, np.float32), np.empty(M, np.float32)
        _lib.check(fn(h, *args, p(off), p(sc)))
        return off, sc

    forms = {
        "parent_host_float": lambda: call(L.vaqhip_learn_quantization, p(Xf), n, 0, ratio),
        "u8_host": lambda: call(L.vaqhip_learn_quantization_u8, p(X8), n, 0, ratio),
        "device_float": lambda: call(L.vaqhip_learn_quantization_device, C.c_void_p(d_f.data_ptr()), n, 0, ratio),
        "refiner_u8": lambda: call(L.vaqhip_learn_quantization_from_refiner, r8._h, ratio),
        "refiner_float": lambda: call(L.vaqhip_learn_quantization_from_refiner, rf._h, ratio),
    }
    for name, f in forms.items():  # warm-up
        with step_limit(a.step_limit, name + " (warm-up)"):
            f()
    t = {k: [] for k in forms}
    phases = {}
    for _ in range(max(a.runs, 5)):
        want = None
        for name, f in forms.items():
            with step_limit(a.step_limit, name):
                t0 = time.perf_counter()
                got = f()
                t[name].append((time.perf_counter() - t0) * 1e3)
            if want is None:
                want = got
                continue
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), name
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), name
            ph = v.last_learn_timing()
            phases[name] = {k: (round(x, 3) if k.endswith("_ms") else x) for k, x in ph.items() if k != "loss"}
    with step_limit(a.step_limit, "u8_device"):  # (untimed: equality only)
        got = call(L.vaqhip_learn_quantization_u8_device, C.c_void_p(d_8.data_ptr()), n, 0, ratio)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    peak = {}
    for name, f in forms.items():
        with step_limit(a.step_limit, name + " (peak bytes)"):
            peak[name] = peak_bytes_during(torch, f)
    res = {k: dict(stats(x), last_phases=phases.get(k)) for k, x in t.items()}
    par = res["parent_host_float"]
    for k, r in res.items():
        if k != "parent_host_float":
            r["faster_than_parent_beyond_the_spread"] = r["max_ms"] < par["min_ms"]
            r["slower_than_parent_beyond_the_spread"] = r["min_ms"] > par["max_ms"]
            r["bit_equal"] = True
    sample = int(np.float32(a.ratio) * np.float32(n))
    out = {"tool": "tools/bench_learn_quantization.py", "source_hash": build.source_hash(),
           "gpu": torch.cuda.get_device_name(0), "gpus_used": 1,
           "workload": f"{n} x {D} byte-valued rows, {M} x 4-bit codes, rotation, ratio {a.ratio} ({sample} sampled rows); "
                       "wall ms of the synchronous call, the five forms in turn, outputs asserted bit-equal to the parent's "
                       "on every repetition",
           "forms": res,
           "device_bytes": {"peak_during_the_call": peak,
                            "how": "free device memory (hipMemGetInfo) before the call minus its lowest sample during one "
                                   "untimed call, sampled by a thread every 0.2 ms; rows resident beforehand not included",
                            "sample_rows_float": sample * D * 4,
                            "plan_group_of_all_columns": sample * 16 * 4 * (M + 4)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {x: r[x] for x in ("median_ms", "min_ms", "max_ms")} for k, r in res.items()}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
