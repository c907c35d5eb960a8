"""The Hamming engine's encoders on the GPU (VaqBitVec.set_encoder / encode / set_rows_encoded / encode_from_refiner and
vaq_amd.bitvec_fit_thresholds over vaqhip_bitvec_*): every word and every threshold bit for bit against the
restatement (tests/bitvec_encode_ref.py) over oracle.project's values.  Rows: two of the kernel's row tiles + 1."""
import numpy as np
import pytest

import bitvec_encode_ref as er
import bitvec_ref as br
from bitvec_cases import crosses
from oracle import pyoracle as po
from vaq_amd import VaqBitVec, VaqHipError, VaqRefiner, bitvec_fit_thresholds, bitvec_fit_thresholds_u8

pytestmark = pytest.mark.gpu
F = np.float32


def rotation(rs, D):
    return np.linalg.qr(rs.standard_normal((D, D)))[0].astype(F)


def raw_rows(rs, n, D, elem):
    return rs.randint(0, 256, (n, D)).astype(np.uint8) if elem == "u8" else (rs.standard_normal((n, D)) * 9).astype(F)


def both_forms(bv, X):
    """encode() of host rows and of a torch tensor on another stream: the same words"""
    import torch
    host = bv.encode(X)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = bv.encode(torch.from_numpy(X).cuda())
    s.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), host)
    return host


@pytest.mark.parametrize("elem", ["f32", "u8"])
@pytest.mark.parametrize("eig", [False, True])
@pytest.mark.parametrize("D", er.SIGN_DIMS)
def test_sign_form(vaqlib, D, eig, elem):
    rs = np.random.RandomState(D)
    X = raw_rows(rs, 2 * er.tile_rows(D) + 1, D, elem)
    if elem == "f32" and not eig:  # projected input: +0, -0, NaN, +-inf, denormals in rows 0..7 of the end columns
        X[:8, 0] = X[:8, D - 1] = er.SPECIALS
    E = rotation(rs, D) if eig else None
    bv = VaqBitVec(0, D)
    bv.set_encoder(D, E)
    Xp = po.project(X.astype(F), E) if eig else X.astype(F)
    assert np.array_equal(both_forms(bv, X), er.sign_ref(Xp))
    bv.close()


@pytest.mark.parametrize("D", [127, 191])
def test_sign_form_refuses_the_shift_by_64(vaqlib, D):
    bv = VaqBitVec(0, D)
    with pytest.raises(VaqHipError) as e:
        bv.set_encoder(D)
    assert e.value.code == -2
    with pytest.raises(VaqHipError) as e:
        bv.encode(np.zeros((1, D), F))
    assert e.value.code == -7  # still no encoder
    bv.close()


@pytest.mark.parametrize("name", er.ALLOCS)
def test_quantile_form(vaqlib, name):
    bits, train, T, rows = er.quantile_case(name)
    D = len(bits)
    bv = VaqBitVec(0, sum(bits))
    bv.set_encoder(D, None, bits, T)  # projected input: the constant column, a threshold, above the range, inf, NaN
    assert np.array_equal(both_forms(bv, rows), er.quantile_ref(rows, bits, T))
    rs = np.random.RandomState(D)
    E, Xb = rotation(rs, D) * F(0.1), raw_rows(rs, len(rows), D, "u8")  # byte rows through the rotation
    bv.set_encoder(D, E, bits, T)
    assert np.array_equal(both_forms(bv, Xb), er.quantile_ref(po.project(Xb.astype(F), E), bits, T))
    for bad_bits, bad_T in ((bits[:-1] + [9], T), (bits[:-1] + [bits[-1] - 1], T), (bits, np.full_like(T, np.nan))):
        with pytest.raises(VaqHipError) as e:  # a bit count outside 0..8, a sum that is not n_bits, a NaN threshold
            bv.set_encoder(D, None, bad_bits, bad_T)
        assert e.value.code == -1
    bv.close()


@pytest.mark.parametrize("elem", ["f32", "u8"])
@pytest.mark.parametrize("n", [4099, 2])
def test_fit_thresholds(vaqlib, n, elem):
    import torch
    rs = np.random.RandomState(n)
    bits, D = [8, 0, 3, 1, 5], 5
    X, E = raw_rows(rs, n, D, elem), rotation(rs, D)
    fit = bitvec_fit_thresholds_u8 if elem == "u8" else bitvec_fit_thresholds
    want = er.thresholds_ref(po.project(X.astype(F), E), bits, fill=7.0)
    got = fit(X, bits, E, out=np.full((D, 256), 7.0, F))  # (7.0: what the fit does not write stays)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = fit(torch.from_numpy(X).cuda(), bits, torch.from_numpy(E).cuda(), out=torch.full((D, 256), 7.0, device="cuda"))
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if elem == "f32":
        X[1, 1] = np.nan  # an unallocated column is never looked at
        assert np.array_equal(fit(X, bits)[2].view(np.uint32), er.thresholds_ref(X, bits)[2].view(np.uint32))
        X[1, 2] = np.nan
        for b, text in ((bits, "NaN"), ([9] + bits[1:], "bits[0]=9")):
            with pytest.raises(VaqHipError) as e:
                fit(X, b)
            assert e.value.code == -1 and text in str(e.value)


@pytest.mark.parametrize("elem", ["f32", "u8"])
@pytest.mark.parametrize("form", ["sign", "quantile"])
def test_end_to_end_query_and_rerank(vaqlib, form, elem):
    """rows made on the device (from a refiner; by set_rows_encoded + add_rows_encoded) and device-encoded queries
    answer as the restatement's bits do after set_rows"""
    import torch
    rs = np.random.RandomState(7)
    D, n, nq, k = 16, 700, 5, 40
    X = rs.randint(0, 256, (30, D))[rs.randint(0, 30, n)].astype(np.uint8 if elem == "u8" else F)  # 30 distinct rows
    XQ, E = X[:nq].astype(F), rotation(rs, D)
    bits = None if form == "sign" else [3, 0] * 8
    Xp, XQp = po.project(X.astype(F), E), po.project(XQ, E)
    T = None if bits is None else er.thresholds_ref(Xp, bits)
    ref = (lambda P: er.sign_ref(P)) if bits is None else (lambda P: er.quantile_ref(P, bits, T))
    rows, queries = ref(Xp), ref(XQp)
    assert crosses(br.hamming_dists(rows, queries[:1])[0], k), "slot k is not inside a crowd of ties"
    want = VaqBitVec(0, D if bits is None else sum(bits))
    want.set_rows(rows, id_base=9)
    r = VaqRefiner(D, 0)
    (r.set_rows_u8 if elem == "u8" else r.set_rows)(X, id_base=9)
    bv = VaqBitVec(0, want.n_bits)
    bv.set_encoder(D, E, bits, T)
    for step in ("refiner", "set_add"):
        if step == "refiner":
            bv.encode_from_refiner(r, id_base=9)
        else:
            bv.set_rows_encoded(X[:33], id_base=9)
            bv.add_rows_encoded(X[33:])
        assert len(bv) == n
        dq, doq = bv.encode(torch.from_numpy(XQ).cuda()), torch.from_numpy(XQ).cuda()
        for got, exp in ((bv.query_device(dq, k), want.query(queries, k)),
                         (bv.query_rerank_device(dq, doq, 10, 4, r), want.query_rerank(queries, XQ, 10, 4, r))):
            assert np.array_equal(got[0].cpu().numpy(), exp[0])
            assert np.array_equal(got[1].cpu().numpy(), exp[1].astype(F))
    for h in (bv, want, r):
        h.close()
