"""The k-means of clusterTI over the shards of a multi-device index, without a GPU: the symbols and the version of
the library, the null-handle refusal, and the host arithmetic that splits the sample over the shards
(vaq_amd/csrc/kmeans_sample.h through tests/cpp/kmeans_split_test.cpp) against tests/kmeans_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import kmeans_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_new_symbols(vaqlib):
    from vaq_amd import _lib
    for name in ("vaqhip_multi_cluster_ti_kmeans", "vaqhip_multi_last_kmeans_timing"):
        assert name in _lib.SYMBOLS and hasattr(vaqlib, name)


def test_version(vaqlib):
    assert vaqlib.vaqhip_version() >= 108


def test_null_handle_is_refused(vaqlib):
    assert vaqlib.vaqhip_multi_cluster_ti_kmeans(None, 4, 1, 50, None, None, None) == -1
    assert vaqlib.vaqhip_multi_last_error()
    assert vaqlib.vaqhip_multi_last_kmeans_timing(None, None) == -1


@pytest.fixture(scope="module")
def split_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kmeans_split") / "kmeans_split_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "vaq_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "kmeans_split_test.cpp"), "-o", exe])
    return exe


def test_nan_rows_header(tmp_path):
    """vaq::nan_rows (kmeans_sample.h), what every k-means here reports of its centres: tests/cpp/nan_rows_test.cpp,
    plain and once more under AddressSanitizer + UBSan (host code only, its own main)."""
    for extra, name in ((["-O2"], "nan_rows_test"),
                        (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "nan_rows_asan")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-I" + os.path.join(ROOT, "vaq_amd", "csrc")] + extra +
                              [os.path.join(ROOT, "tests", "cpp", "nan_rows_test.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "nan_rows_test: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


# N = 9 over 4 shards (one empty); N = 4001 over 3 after an append of 1001 rows; a sampled case (2560 of 20000)
@pytest.mark.parametrize("N,T,G,appended", [(9, 4, 4, 0), (4001, 24, 3, 1001), (20000, 10, 5, 0), (20000, 10, 3, 7000)])
def test_sample_split_over_the_shards(split_exe, N, T, G, appended):
    r = subprocess.run([split_exe, str(N), str(T), str(G), str(appended)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("kmeans_split ok"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    want = kr.sample_rows(N, T)
    rows = len(want)
    assert rows == min(N, kr.ROWS_PER_CENTRE * T)
    # the shards as set_codes cuts them, the appended rows on the last one
    first = N - appended
    per = (first + G - 1) // G
    lo = [min(first, g * per) for g in range(G)]
    n = [min(first, (g + 1) * per) - lo[g] for g in range(G)]
    n[-1] += appended
    got = np.array([[int(x) for x in ln.split()] for ln in lines[:rows]], np.int64)
    assert np.array_equal(got[:, 0], np.arange(rows)) and np.array_equal(got[:, 1], want)
    for pos, row, g, local in got:
        assert lo[g] <= row < lo[g] + n[g] and local == row - lo[g]  # exactly one shard: they do not overlap
    slices = [[int(x) for x in ln.split()[1:]] for ln in lines[rows:rows + G]]
    step = (rows + G - 1) // G
    assert slices == [[g, min(rows, g * step), min(rows, (g + 1) * step)] for g in range(G)]
