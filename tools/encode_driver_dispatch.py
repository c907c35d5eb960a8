#!/usr/bin/env python3
"""Dispatch identity of the single index's encode entries across two builds of the library.

  run <dir>             call vaqhip_encode{,_lut}{,_u8}{,_device} on 300 rows of D = 16 -- every entry with and
                        without a rotation and with projected 0 and 1, the VAQ rule on a grouped-sum and on a
                        sequential-sum index, the LUT rule on the sequential-sum one -- and write the codes of every
                        case to <dir>/codes.npz.  A one-element torch fill in front of every case marks it in a
                        kernel trace.  Meant to run under `rocprofv3 --kernel-trace --stats --output-format csv
                        -d <dir>/kt -- python3 tools/encode_driver_dispatch.py run <dir>`, once per library
                        (VAQHIP_LIB names the one to load).
  compare <dirA> <dirB> per case: the number of dispatches and whether the ordered (kernel name, grid, workgroup,
                        LDS bytes) sequences and the codes are identical; profiles/encode_driver_dispatch.txt is
                        this command's output.
"""
import csv
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, D = 300, 16
SHAPE_COLS = ("LDS_Block_Size", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "Grid_Size_X", "Grid_Size_Y",
              "Grid_Size_Z")


def case_names():
    for index in ("grouped", "sequential", "lut"):
        for rot in (0, 1):
            for projected in (0, 1):
                for form in ("host", "host_u8", "device", "device_u8"):
                    yield f"{index}_rot{rot}_projected{projected}_{form}", index, rot, projected, form


def run(out_dir: str) -> None:
    import torch
    import vaq_amd
    rng = np.random.default_rng(16)
    X8 = rng.integers(0, 256, size=(N, D), dtype=np.uint8)
    Xf = X8.astype(np.float32)
    rotation = np.linalg.qr(rng.normal(size=(D, D)))[0].astype(np.float32)
    d_Xf, d_X8 = torch.from_numpy(Xf).cuda(), torch.from_numpy(X8).cuda()
    marker = torch.zeros(1, device="cuda")
    indexes = {}
    for index in ("grouped", "sequential", "lut"):
        for rot in (0, 1):
            v = vaq_amd.VaqHip(sequential_sum=index != "grouped")
            v.mEigenVectors = rotation if rot else None
            if index == "grouped":
                v.mBitsAlloc = [6, 4, 3, 1]
                v.mCentroidsPerSubs = [(rng.normal(size=(1 << b, 4)) * 60 + 128).astype(np.float32) for b in v.mBitsAlloc]
            else:
                v.mBitsAlloc = [1 + d % 4 for d in range(D)]
                v.fitQuantiles(Xf)
            indexes[index, rot] = v
    torch.cuda.synchronize()
    codes = {}
    for name, index, rot, projected, form in case_names():
        v = indexes[index, rot]
        lut = index == "lut"
        marker.fill_(0)
        if form == "host":
            (v.encodeLUT if lut else v.encode)(Xf, projected=bool(projected))
            got = v.mCodebook
        elif form == "host_u8":
            (v.encodeLUT_u8 if lut else v.encode_u8)(X8, projected=bool(projected))
            got = v.mCodebook
        elif form == "device":
            got = (v.encodeLUT_device if lut else v.encode_device)(d_Xf, projected=bool(projected)).cpu().numpy()
        else:
            got = (v.encodeLUT_u8_device if lut else v.encode_u8_device)(d_X8, projected=bool(projected)).cpu().numpy()
        torch.cuda.synchronize()
        codes[name] = np.array(got).view(np.uint16)
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, "codes.npz"), **codes)
    print(f"{len(codes)} cases, library {vaq_amd.lib_path()}")


def case_sequences(run_dir: str):
    """The kernel trace under run_dir cut at the markers: one list of (name, shape...) per case, setup dropped."""
    files = glob.glob(os.path.join(run_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Dispatch_Id"]))
    cases, cur = [], None
    for r in rows:
        if "at::native" in r["Kernel_Name"]:
            cur = []
            cases.append(cur)
        elif cur is not None:
            cur.append((r["Kernel_Name"],) + tuple(int(r[c]) for c in SHAPE_COLS))
    return cases[1:]  # (the first fill is the marker's own torch.zeros)


def short_name(kernel: str) -> str:
    """project_kernel of "void vaq::(anonymous namespace)::project_kernel<float>(...)"."""
    m = re.search(r"(\w+)\s*(<|\(|$)", kernel.replace("(anonymous namespace)::", "").replace("void ", ""))
    return m.group(1) if m else kernel


def compare(dir_a: str, dir_b: str) -> int:
    names = [c[0] for c in case_names()]
    seq_a, seq_b = case_sequences(dir_a), case_sequences(dir_b)
    assert len(seq_a) == len(names) == len(seq_b), (len(seq_a), len(seq_b), len(names))
    codes_a, codes_b = np.load(os.path.join(dir_a, "codes.npz")), np.load(os.path.join(dir_b, "codes.npz"))
    print("# ordered (kernel name, grid, workgroup, LDS bytes) of every dispatch of an encode entry, parent library against")
    print(f"# this tree's (rocprofv3 --kernel-trace, columns {', '.join(SHAPE_COLS)}); codes = the {N} x M uint16 matrix")
    print("# [kernels of the sequence, the runtime's buffer copies left out of this list only]")
    bad = 0
    for name, a, b in zip(names, seq_a, seq_b):
        same_seq, same_codes = a == b, np.array_equal(codes_a[name], codes_b[name])
        bad += not (same_seq and same_codes and a)
        kernels = " ".join(short_name(k[0]) for k in b if "copyBuffer" not in k[0])
        print(f"{name:44s} dispatches {len(a):3d} / {len(b):3d}  sequence {'identical' if same_seq else 'DIFFERENT'}  "
              f"codes {'identical' if same_codes else 'DIFFERENT'}  [{kernels}]")
    print("verdict: all cases identical" if not bad else f"verdict: {bad} cases differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
