"""Build the gfx950 shared library (vaq_amd/lib/libvaqhip.so) with hipcc.

hipcc cross-compiles for gfx950 without a GPU.  -ffp-contract=off is part of
the numerics contract (vaq_kernels.hip header): only explicit fmaf() fuses.
"""
from __future__ import annotations

import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vaq_amd", "csrc")
LIBDIR = os.path.join(ROOT, "vaq_amd", "lib")
LIB = os.path.join(LIBDIR, "libvaqhip.so")
SOURCES = ["vaq_kernels.hip", "vaq_scan_bytes.hip", "vaq_scan_bits.hip", "vaq_scan_bf.hip", "vaq_scan_bm.hip", "vaq_exact.hip", "vaq_ti.hip", "vaq_kmeans.hip", "vaq_codebooks.hip", "vaq_fast.hip", "vaq_lutfit.hip", "vaq_learn.hip", "vaq_refine.hip", "vaq_exhaust.hip", "vaq_train.hip", "vaqhip_api.cpp", "vaqhip_plan.cpp", "vaqhip_search.cpp", "vaqhip_codes.cpp", "vaqhip_fast.cpp", "vaqhip_learn.cpp", "vaqhip_lutfit.cpp", "vaqhip_codebooks.cpp", "vaqhip_train.cpp", "vaqhip_refiner.cpp",
           "vaqhip_multi.cpp", "vaqhip_multi_search.cpp", "vaqhip_multi_kmeans.cpp", "vaqhip_multi_refiner.cpp", "vaqhip_multi_refiner_search.cpp", "vaqhip_multi_encode.cpp", "vaqhip_multi_lutfit.cpp", "vaqhip_multi_learn.cpp", "vaqhip_multi_codebooks.cpp", "vaqhip_rccl.cpp"]
MULTI_REFINER_SOURCES = ("vaqhip_multi_refiner.cpp", "vaqhip_multi_refiner_search.cpp")
MULTI_ENCODE_SOURCE = "vaqhip_multi_encode.cpp"  # reads the multi refiner's resident rows: its headers too
MULTI_LUTFIT_SOURCE = "vaqhip_multi_lutfit.cpp"  # the sharded quantile fit: reads the multi refiner's resident rows too
MULTI_LEARN_SOURCE = "vaqhip_multi_learn.cpp"  # learnQuantization over the multi refiner's resident rows
MULTI_CODEBOOKS_SOURCE = "vaqhip_multi_codebooks.cpp"  # the sharded codebook fit: reads the multi refiner's resident rows too
MULTI_SOURCES = ("vaqhip_multi.cpp", "vaqhip_multi_search.cpp", "vaqhip_multi_kmeans.cpp", MULTI_ENCODE_SOURCE, MULTI_LUTFIT_SOURCE, MULTI_LEARN_SOURCE, MULTI_CODEBOOKS_SOURCE) + MULTI_REFINER_SOURCES
KERNEL_HEADER = os.path.join(CSRC, "vaq_kernels.h")
OWNER_HEADER = os.path.join(CSRC, "refine_owner.h")  # the refiner's cut and label -> shard: vaq_kernels.h brings it
API_HEADER = os.path.join(ROOT, "include", "vaqhip.h")


SCAN_HEADER = os.path.join(CSRC, "vaq_scan.h")
SCAN_BF_HEADER = os.path.join(CSRC, "vaq_scan_bf.h")
FAST_HEADER = os.path.join(CSRC, "vaq_fast.h")
REFINE_GROUP_HEADER = os.path.join(CSRC, "vaq_refine_group.h")  # Eigen's squaredNorm over 16 lanes: refine, exhaustive form
EXHAUST_HEADER = os.path.join(CSRC, "vaq_exhaust.h")  # the same by one thread, host and device: exhaustive form
EXHAUST_PLAN_HEADER = os.path.join(CSRC, "vaqhip_exhaust_plan.h")  # the exhaustive form's plan and launches: both refiners
REFINE_COMMON_HEADER = os.path.join(CSRC, "vaqhip_refine_common.h")  # checks, options, the row store: both refiners
MULTI_REFINER_HEADER = os.path.join(CSRC, "vaqhip_multi_refiner.h")  # private to the multi refiner's two host files
SHARD_RUN_HEADER = os.path.join(CSRC, "vaqhip_shard_run.h")  # the call-owned run and its teardown: the sharded builds
RESTATED_HEADER = os.path.join(CSRC, "vaq_restated.h")  # stdsort, stdheap, refheap, sq_norm_eigen: FAST, TI planning, the replay, k-means, refine
INTERNAL_HEADER = os.path.join(CSRC, "vaqhip_internal.h")
INDEX_HEADER = os.path.join(CSRC, "vaqhip_index.h")  # private to the single-index host files
DEV_HEADER = os.path.join(CSRC, "vaqhip_dev.h")      # DevBuf, DeviceGuard: both hosts and the scratch allocators
MULTI_HEADER = os.path.join(CSRC, "vaqhip_multi.h")  # private to the multi-device host files; brings the next two
JOB_POOL_HEADER = os.path.join(CSRC, "job_pool.h")
RCCL_HEADER = os.path.join(CSRC, "vaqhip_rccl.h")
KMEANS_SAMPLE_HEADER = os.path.join(CSRC, "kmeans_sample.h")  # the k-means' sample and its split: both hosts
LUTFIT_HEADER = os.path.join(CSRC, "vaq_lutfit.h")  # binaryEncodingLUT's two lambdas: kernels and host
LUTFIT_DEV_HEADER = os.path.join(CSRC, "vaq_lutfit_dev.h")  # the column fit's two halves: kernels and the sharded fit
LUTFIT_PLAN_HEADER = os.path.join(CSRC, "lutfit_multi_plan.h")  # owners, rounds, offsets of the sharded fit (no HIP)
LEARN_PLAN_HEADER = os.path.join(CSRC, "learn_plan.h")  # learnQuantization's host arithmetic: both forms, the loss kernel (no HIP)
LEARN_HEADER = os.path.join(CSRC, "vaq_learn.h")  # the kernels of learnQuantization's device forms
CODEBOOKS_PLAN_HEADER = os.path.join(CSRC, "fit_codebooks_plan.h")  # samples, offsets, key width of the codebook fit (no HIP)
TRAIN_PLAN_HEADER = os.path.join(CSRC, "train_plan.h")  # sample, plan and exact bit allocation of the training front half (no HIP)
TRAIN_ROT_HEADER = os.path.join(CSRC, "vaq_train_rot.h")  # the Jacobi rotation, ordering and host solver: kernels and host
TRAIN_HEADER = os.path.join(CSRC, "vaq_train.h")  # the kernels of the training front half
CODEBOOKS_MULTI_PLAN_HEADER = os.path.join(CSRC, "fit_codebooks_multi_plan.h")  # owners, sub-plans, sample split of the sharded fit (no HIP)
CODEBOOKS_HIER_PLAN_HEADER = os.path.join(CSRC, "fit_codebooks_hier_plan.h")  # rows, batches, refusals, tiles of the hierarchical fit (no HIP)
CODEBOOKS_BIN_PLAN_HEADER = os.path.join(CSRC, "fit_codebooks_bin_plan.h")  # nodes, level batches, chunks, tiles of the binary-tree fit (no HIP)


def _deps(src: str):
    # only the host files see the public C header; the scan bodies live in vaq_scan.h
    deps = [os.path.join(CSRC, src), KERNEL_HEADER, OWNER_HEADER]
    if src == "vaqhip_rccl.cpp":  # nothing of the index
        return [os.path.join(CSRC, src), RCCL_HEADER]
    if src.endswith(".cpp"):
        deps += [API_HEADER, INTERNAL_HEADER, DEV_HEADER]
        deps += [MULTI_HEADER, JOB_POOL_HEADER, RCCL_HEADER] if src in MULTI_SOURCES else [INDEX_HEADER]
    if src in ("vaq_kernels.hip", "vaq_ti.hip", "vaq_kmeans.hip", "vaq_lutfit.hip", "vaq_codebooks.hip"):
        deps.append(DEV_HEADER)
    if src in ("vaq_codebooks.hip", "vaqhip_codebooks.cpp", MULTI_CODEBOOKS_SOURCE):
        deps += [CODEBOOKS_PLAN_HEADER, KMEANS_SAMPLE_HEADER]
    if src in ("vaq_codebooks.hip", "vaqhip_codebooks.cpp"):
        deps.append(CODEBOOKS_HIER_PLAN_HEADER)
        deps.append(CODEBOOKS_BIN_PLAN_HEADER)
    if src == MULTI_CODEBOOKS_SOURCE:
        deps.append(CODEBOOKS_MULTI_PLAN_HEADER)
    if src in ("vaq_train.hip", "vaqhip_train.cpp"):
        deps += [TRAIN_PLAN_HEADER, TRAIN_ROT_HEADER, TRAIN_HEADER, KMEANS_SAMPLE_HEADER]
    if src in ("vaq_lutfit.hip", "vaqhip_lutfit.cpp", MULTI_LUTFIT_SOURCE, "vaq_learn.hip"):
        deps.append(LUTFIT_HEADER)
    if src in ("vaq_learn.hip", "vaqhip_learn.cpp", "vaqhip_fast.cpp"):
        deps.append(LEARN_PLAN_HEADER)
    if src in ("vaq_learn.hip", "vaqhip_learn.cpp", MULTI_LEARN_SOURCE):
        deps.append(LEARN_HEADER)
    if src in ("vaq_lutfit.hip", MULTI_LUTFIT_SOURCE):
        deps.append(LUTFIT_DEV_HEADER)
    if src == MULTI_LUTFIT_SOURCE:
        deps.append(LUTFIT_PLAN_HEADER)
    if src in ("vaq_kmeans.hip", "vaqhip_codes.cpp", "vaqhip_multi_kmeans.cpp", "vaqhip_learn.cpp", MULTI_LEARN_SOURCE):
        deps.append(KMEANS_SAMPLE_HEADER)
    if src in ("vaq_kernels.hip", "vaq_scan_bytes.hip", "vaq_scan_bits.hip", "vaq_scan_bf.hip", "vaq_scan_bm.hip", "vaq_exact.hip", "vaq_refine.hip", "vaq_exhaust.hip"):
        deps.append(SCAN_HEADER)
    if src in ("vaq_kernels.hip", "vaq_scan_bf.hip", "vaq_scan_bm.hip"):
        deps.append(SCAN_BF_HEADER)
    if src in ("vaq_fast.hip", "vaqhip_fast.cpp"):
        deps.append(FAST_HEADER)
    if src in ("vaq_fast.hip", "vaqhip_fast.cpp", "vaq_exact.hip", "vaq_ti.hip", "vaq_kmeans.hip", "vaq_codebooks.hip", "vaq_refine.hip", "vaq_exhaust.hip"):
        deps.append(RESTATED_HEADER)
    if src in ("vaq_refine.hip", "vaq_exhaust.hip"):
        deps.append(REFINE_GROUP_HEADER)
    if src == "vaq_exhaust.hip":
        deps.append(EXHAUST_HEADER)
    if src == "vaqhip_refiner.cpp" or src in MULTI_REFINER_SOURCES or src in (MULTI_ENCODE_SOURCE, MULTI_LUTFIT_SOURCE, MULTI_LEARN_SOURCE, MULTI_CODEBOOKS_SOURCE):
        deps += [EXHAUST_PLAN_HEADER, REFINE_COMMON_HEADER]
    if src in MULTI_REFINER_SOURCES or src in (MULTI_ENCODE_SOURCE, MULTI_LUTFIT_SOURCE, MULTI_LEARN_SOURCE, MULTI_CODEBOOKS_SOURCE):
        deps.append(MULTI_REFINER_HEADER)
    if src in (MULTI_ENCODE_SOURCE, MULTI_LUTFIT_SOURCE, MULTI_LEARN_SOURCE, MULTI_CODEBOOKS_SOURCE):
        deps.append(SHARD_RUN_HEADER)
    return deps
OBJDIR = os.path.join(LIBDIR, "obj")
# Experiment builds: VAQ_VARIANT=name compiles (with VAQ_EXTRA_FLAGS) into vaq_amd/lib/variants/name/
# and VAQHIP_LIB=<path> makes the package load that library instead (tools/ sweeps).
_VARIANT = os.environ.get("VAQ_VARIANT", "")
# VAQ_VARIANT_ONLY="a.hip b.hip": only these units are compiled with the variant's flags, the
# others are linked from the main build's objects (which must be up to date)
_VARIANT_ONLY = os.environ.get("VAQ_VARIANT_ONLY", "").split()
_MAIN_OBJDIR = OBJDIR
if _VARIANT:
    LIBDIR = os.path.join(LIBDIR, "variants", _VARIANT)
    LIB = os.path.join(LIBDIR, "libvaqhip.so")
    OBJDIR = os.path.join(LIBDIR, "obj")


def _flags_tag() -> str:
    return os.environ.get("VAQ_EXTRA_FLAGS", "")


def _obj(src: str) -> str:
    d = OBJDIR
    if _VARIANT and _VARIANT_ONLY and src not in _VARIANT_ONLY:
        d = _MAIN_OBJDIR
    return os.path.join(d, os.path.splitext(src)[0] + ".o")


def _obj_stale(src: str) -> bool:
    o = _obj(src)
    if not os.path.exists(o):
        return True
    t = os.path.getmtime(o)
    tag = o + ".flags"
    if not os.path.exists(tag) or open(tag).read() != _flags_tag():
        return True
    return any(os.path.getmtime(d) > t for d in _deps(src))


def build_lib(force: bool = False, verbose: bool = False) -> str:
    """Compile each translation unit to an object (in parallel, only the stale
    ones) and link them into libvaqhip.so."""
    if os.environ.get("VAQHIP_LIB") and not _VARIANT:
        return os.environ["VAQHIP_LIB"]  # a prebuilt experiment library was named: leave it alone
    if os.environ.get("VAQ_NO_BUILD"):
        # under rocprofv3 a child process (hipcc -> clang) is the exec-after-GPU-init hop the pool
        # forbids: the library must have been built beforehand (tools/profile_*.sh do that)
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " is missing and VAQ_NO_BUILD is set: run `python -m vaq_amd.build` first")
        return LIB
    os.makedirs(OBJDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
              "-ffp-contract=off", "-fno-fast-math", "-Wall",
              "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    extra = _flags_tag().split()
    todo = [s for s in SOURCES if (force or _obj_stale(s)) and
            not (_VARIANT and _VARIANT_ONLY and s not in _VARIANT_ONLY)]
    procs = []
    for s in todo:
        cmd = common + extra + ["-c", os.path.join(CSRC, s), "-o", _obj(s)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((s, cmd, subprocess.Popen(cmd)))
    failed = [s for s, _, p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, "hipcc -c " + " ".join(failed))
    for s in todo:
        with open(_obj(s) + ".flags", "w") as f:
            f.write(_flags_tag())
    objs = [_obj(s) for s in SOURCES]
    if todo or not os.path.exists(LIB) or any(os.path.getmtime(o) > os.path.getmtime(LIB) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl", "-lpthread"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return LIB


def source_hash() -> str:
    """Identity of the library's sources (csrc + include): profile files under profiles/ carry it, and
    bench.py only attaches their counter figures to a run of the SAME build."""
    import hashlib
    h = hashlib.sha1()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp")))
    files += sorted(os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include")))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def build_demo(force: bool = False) -> str:
    """examples/demo_vaqhip.cpp: plain g++ against the C ABI (no hipcc needed)."""
    lib = build_lib()
    out_dir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "demo_vaqhip")
    src = os.path.join(ROOT, "examples", "demo_vaqhip.cpp")
    hdrs = [os.path.join(ROOT, "include", h) for h in ("vaqhip.h", "vaqhip.hpp", "vaqhip_io.hpp")]
    if not force and os.path.exists(exe) and all(
            os.path.getmtime(f) <= os.path.getmtime(exe) for f in [src, lib] + hdrs):
        return exe
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
           src, "-o", exe, "-L" + LIBDIR, "-lvaqhip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose=True))
