"""What the Python adapter of the two refiners refuses before it calls the library: VaqRefiner and VaqMultiRefiner
share these checks through one base class (vaq_amd/refiner.py), and each must raise VaqHipError(-1, ...) with the
text it always had.  Constructing a refiner creates its C object, hence the gpu mark; no refusal reaches a kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, N = 8, 16


@pytest.fixture(scope="module", params=["single", "multi"])
def refiner(request, vaqlib):
    import vaq_amd
    r = vaq_amd.VaqRefiner(D) if request.param == "single" else vaq_amd.VaqMultiRefiner([0, 0], D)
    r.set_rows(np.arange(N * D, dtype=np.float32).reshape(N, D))
    yield r
    r.close()


def refused(call, text):
    from vaq_amd import VaqHipError
    with pytest.raises(VaqHipError) as e:
        call()
    assert e.value.code == -1
    assert str(e.value) == f"vaqhip error -1 (EINVAL): {text}"


@pytest.mark.parametrize("method", ["set_rows", "add_rows", "search", "refine"])
def test_wrong_D_is_refused_with_the_rows_text(refiner, method):
    X = np.zeros((3, D + 1), np.float32)
    args = {"search": (X, 1), "refine": (X, np.zeros(3, np.int32), 1)}.get(method, (X,))
    refused(lambda: getattr(refiner, method)(*args), f"rows (3, {D + 1}) are not n x {D}")
    refused(lambda: getattr(refiner, method)(*((np.zeros(D, np.float32),) + args[1:])), f"rows ({D},) are not n x {D}")


@pytest.mark.parametrize("method", ["set_rows_u8", "add_rows_u8"])
def test_anything_but_contiguous_uint8_rows_is_refused_by_the_u8_forms(refiner, method):
    text = f"byte rows must be a contiguous uint8 n x {D} array (nothing is converted)"
    for X in (np.zeros((3, D), np.float32), np.zeros((3, D), np.int8), np.zeros((3, D + 1), np.uint8),
              np.zeros((3, 2 * D), np.uint8)[:, ::2], np.zeros(D, np.uint8)):
        refused(lambda: getattr(refiner, method)(X), text)
    assert refiner.elem_size == 4  # (nothing replaced the float rows)


def test_label_count_that_nq_does_not_divide_is_refused(refiner):
    from vaq_amd import LabelDistVec
    X = np.zeros((3, D), np.float32)
    refused(lambda: refiner.refine(X, np.zeros(7, np.int32), 1), "7 labels for 3 queries")
    refused(lambda: refiner.refine(X, LabelDistVec(np.zeros(10, np.int32), np.zeros(10, np.float32)), 2),
            "10 labels for 3 queries")
    ans = refiner.refine(X, np.zeros(6, np.int32), 1)  # 6 = 3 x 2 passes the same check
    assert ans.labels.shape == (3,) and (ans.labels == 0).all()
