"""The CPU side of the Hamming engine's encoders: the header the kernels run (vaq_amd/csrc/vaq_bitvec_encode.h), built for the host, equals tests/bitvec_encode_ref.py bit for bit
(tests/cpp/bitvec_encode_test.cpp, once more under AddressSanitizer + UBSan: host code only, its own main)."""
import os
import shutil
import subprocess

import numpy as np

import bitvec_encode_ref as er


def sign_rows(D):
    rs = np.random.RandomState(D)
    X = rs.standard_normal((2 * er.tile_rows(D) + 1, D)).astype(np.float32)
    X[:8, 0] = X[:8, D - 1] = er.SPECIALS
    return X


def test_shared_header_matches_the_restatement(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        np.array([len(er.SIGN_DIMS) + len(er.ALLOCS)], np.int32).tofile(f)
        for D in er.SIGN_DIMS:
            X = sign_rows(D)
            for a in (np.array([len(X), D, 0, 0] + [1] * D, np.int32), X, er.sign_ref(X)):
                np.ascontiguousarray(a).tofile(f)
        for name in er.ALLOCS:
            bits, train, T, rows = er.quantile_case(name)
            for a in (np.array([len(rows), len(bits), 1, len(train)] + bits, np.int32), rows, train, T,
                      er.quantile_ref(rows, bits, T)):
                np.ascontiguousarray(a).tofile(f)
    for extra, name in ((["-O2"], "bitvec_encode_test"),
                        (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "bitvec_encode_asan")):
        exe = str(tmp_path / name)
        subprocess.check_call([shutil.which("g++"), "-std=c++17", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                               "-I" + os.path.join(root, "vaq_amd", "csrc")] + extra +
                              [os.path.join(root, "tests", "cpp", "bitvec_encode_test.cpp"), "-o", exe])
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "bitvec_encode_test: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
