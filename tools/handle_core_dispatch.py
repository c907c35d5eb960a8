#!/usr/bin/env python3
"""Dispatch identity of one call on each single-device handle across two builds of the library.

  run <dir>             one call each of the index's search, the FAST search, the refiner's refine, the fused
                        search + refine, the exhaustive search, the Hamming query and its rerank (host forms: staging,
                        workspace scope and launches), on 3000 rows of D = 32 and 70 queries; the answers go to
                        <dir>/answers.npz.  A one-element torch fill in front of every case marks it in a kernel
                        trace.  Meant to run under `rocprofv3 --kernel-trace --output-format csv -d <dir>/kt --
                        python3 tools/handle_core_dispatch.py run <dir>`, once per library (VAQHIP_LIB names the one
                        to load).
  compare <dirA> <dirB> per case: the number of dispatches and whether the ordered (kernel name, grid, workgroup,
                        LDS bytes) sequences and the answers are identical; profiles/handle_core_dispatch.txt is this
                        command's output.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from encode_driver_dispatch import SHAPE_COLS, case_sequences, short_name  # noqa: E402  (the trace reader)

N, D, NQ, K, R = 3000, 32, 70, 10, 40
CASES = ("index_search", "fast_search", "refiner_refine", "fused_search_refine", "exhaustive_search", "bitvec_query",
         "bitvec_rerank")


def run(out_dir: str) -> None:
    import torch
    import vaq_amd
    from helpers import make_case
    rng = np.random.default_rng(32)
    c, cf = make_case(7, D, [8] * 8, N, NQ), make_case(8, D, [4] * 8, N, NQ)
    v, f = vaq_amd.VaqHip(device=0), vaq_amd.VaqHipFast(device=0)
    f.parseMethodString("VAQ32m8min1max4var1,FAST")
    for x, case in ((v, c), (f, cf)):
        x.mBitsAlloc, x.mCentroidsPerSubs, x.mEigenVectors, x.mCodebook = case["bits"], case["cents"], case["eig"], case["codes"]
    f.setLUTQuantization(np.zeros(8, np.float32), np.full(8, 0.01, np.float32))
    v._ensure_codes()
    f._ensure_codes()
    base = rng.integers(0, 256, size=(N, D)).astype(np.float32)
    r = vaq_amd.VaqRefiner(D)
    r.set_rows(base)
    bits = rng.integers(0, 2**63, size=(N, 2), dtype=np.uint64)
    bq = rng.integers(0, 2**63, size=(NQ, 2), dtype=np.uint64)
    bv = vaq_amd.VaqBitVec(0, 128)
    bv.set_rows(bits)
    cand = rng.integers(0, N, size=(NQ, R)).astype(np.int32)
    pair = lambda a: (a.labels, a.distances) if hasattr(a, "labels") else tuple(np.asarray(t) for t in a)
    calls = {
        "index_search": lambda: v.search(c["X"], K),
        "fast_search": lambda: f.search(cf["X"], K),
        "refiner_refine": lambda: r.refine(c["X"], cand, K),
        "fused_search_refine": lambda: v.search_refine(c["X"], R, K, r),
        "exhaustive_search": lambda: r.search(c["X"], K),
        "bitvec_query": lambda: bv.query(bq, K),
        "bitvec_rerank": lambda: bv.query_rerank(bq, c["X"], K, 4, r),
    }
    marker = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    answers = {}
    for name in CASES:
        marker.fill_(0)
        lab, dis = pair(calls[name]())
        torch.cuda.synchronize()
        answers[name + "_labels"], answers[name + "_distances"] = np.array(lab), np.array(dis)
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, "answers.npz"), **answers)
    print(f"{len(CASES)} cases, library {vaq_amd.lib_path()}")


def compare(dir_a: str, dir_b: str) -> int:
    seq_a, seq_b = case_sequences(dir_a), case_sequences(dir_b)
    assert len(seq_a) == len(CASES) == len(seq_b), (len(seq_a), len(seq_b))
    ans_a, ans_b = np.load(os.path.join(dir_a, "answers.npz")), np.load(os.path.join(dir_b, "answers.npz"))
    print("# ordered (kernel name, grid, workgroup, LDS bytes) of every dispatch of one call per handle and form, parent library")
    print(f"# against this tree's (rocprofv3 --kernel-trace, columns {', '.join(SHAPE_COLS)}); answers = labels and distances byte for byte")
    print("# [kernels of the sequence, the runtime's buffer copies left out of this list only]")
    bad = 0
    for name, a, b in zip(CASES, seq_a, seq_b):
        same_seq = a == b
        same_ans = all(ans_a[name + s].tobytes() == ans_b[name + s].tobytes() for s in ("_labels", "_distances"))
        bad += not (same_seq and same_ans and a)
        kernels = " ".join(short_name(k[0]) for k in b if "copyBuffer" not in k[0])
        print(f"{name:22s} dispatches {len(a):3d} / {len(b):3d}  sequence {'identical' if same_seq else 'DIFFERENT'}  "
              f"answers {'identical' if same_ans else 'DIFFERENT'}  [{kernels}]")
    print("verdict: all cases identical" if not bad else f"verdict: {bad} cases differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
