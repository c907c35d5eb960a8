"""The refusals of vaqhip_refiner_fit_centres that are made before the handle is looked into, and the restatement's own
root case; no device.  (A seed out of range, an empty refiner and a NaN row need a refiner: tests/test_kmeans_fit_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import kmeans_fit_ref as kr

P = C.c_void_p(64)  # never dereferenced on these paths


@pytest.mark.parametrize("change,code", [(dict(r=None), -1), (dict(seeds=None), -1), (dict(cen=None), -1), (dict(idx=None), -1),
                                         (dict(it=None), -1), (dict(T=0), -1), (dict(T=4097), -2), (dict(max_iter=0), -1)])
@pytest.mark.parametrize("device_form", [False, True])
def test_refusals(vaqlib, change, code, device_form):
    a = dict(r=P, T=4, seeds=P, max_iter=25, cen=P, idx=P, it=P)
    a.update(change)
    args = [a["r"], a["T"], a["seeds"], a["max_iter"], a["cen"], a["idx"], a["it"]]
    fn = vaqlib.vaqhip_refiner_fit_centres_device if device_form else vaqlib.vaqhip_refiner_fit_centres
    assert fn(*(args + [None] if device_form else args)) == code
    assert vaqlib.vaqhip_last_error()


def test_root_case_needs_the_root():
    X, seeds = kr.root_case()
    with_root, without = kr.fit(X, seeds, 1)[1], kr.fit(X, seeds, 1, root=False)[1]
    assert with_root[2] == 0 and without[2] == 1
    assert np.float32(1) + np.float32(X[0, 1] * X[0, 1]) == np.float32(1 + 2.0 ** -23)
