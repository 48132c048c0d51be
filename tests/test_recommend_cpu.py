"""CPU-only: the recommendation lists' surface exists -- header, library exports, binding, public function -- and the public
function's argument errors are raised before the library is touched.  (What the lists hold is tests/test_hip_recommend.py's.)"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rm_recommend_f32", "rm_recommend_f64", "rm_recommend_dev_f32", "rm_recommend_dev_f64")


def _header():
    text = open(os.path.join(ROOT, "include", "recometrics_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_four_entries():
    text = _header()
    for sym in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % sym, text)
        assert decl, "not declared: " + sym
        args = decl.group(1)
        real = "float" if sym.endswith("f32") else "double"
        for piece in ("Xexcl_csr_p", "Xexcl_csr_i", "int32_t k_top", "int32_t *idx", real + " *score", "int32_t *status"):
            assert piece in args, (sym, piece)
        assert ("int64_t nnz_excl" in args and "void *stream" in args) == ("_dev_" in sym), sym


def test_library_exports_and_binding_lists_them():
    import ctypes
    from recometrics_amd import _binding
    from recometrics_amd import build as rb
    lib = ctypes.CDLL(rb.build())
    for sym in ENTRIES:
        assert hasattr(lib, sym), "missing export: " + sym
        assert sym in _binding.EXPORTS
    assert callable(_binding.recommend) and callable(_binding.recommend_device)


def test_public_function_is_exported():
    import recometrics_amd
    assert "recommend_topk" in recometrics_amd.__all__
    assert callable(recometrics_amd.recommend_topk)
    # the existing surface is still there
    assert {"calc_reco_metrics", "split_reco_train_test"} <= set(recometrics_amd.__all__)


@pytest.fixture
def untouched_library(monkeypatch):
    """any call into the library's recommend entry fails the test: the argument errors must come first"""
    from recometrics_amd import _binding

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_binding, "recommend", boom)
    monkeypatch.setattr(_binding, "load", boom)


def test_argument_errors_come_before_the_library(untouched_library):
    from scipy.sparse import csr_array
    from recometrics_amd import recommend_topk
    A = np.ones((4, 3), np.float32)
    B = np.ones((6, 3), np.float32)
    with pytest.raises(ValueError, match="'k' should be smaller than the number of items."):
        recommend_topk(A, B, k=7)
    with pytest.raises(ValueError, match="'A' and 'B' must have the same number of columns."):
        recommend_topk(A, np.ones((6, 2), np.float32), k=2)
    with pytest.raises(ValueError, match="Must pass item biases if not passing factors."):
        recommend_topk(None, None, k=2)
    with pytest.raises(ValueError, match="passed together"):
        recommend_topk(A, None, k=2)
    with pytest.raises(ValueError, match="Number of items in 'B' and 'X_train' does not match."):
        recommend_topk(A, B, k=2, X_train=csr_array((4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="Number of users in 'A' and 'X_train' does not match."):
        recommend_topk(A, B, k=2, X_train=csr_array((3, 6), dtype=np.float32))
    for bad in ([0, 4], [-1], [1.5]):
        with pytest.raises(ValueError, match="'users'"):
            recommend_topk(A, B, k=2, users=np.array(bad))
    with pytest.raises(ValueError, match="'k' must be positive."):
        recommend_topk(A, B, k=0)


def test_no_users_asked_for_is_an_empty_answer(untouched_library):
    from recometrics_amd import recommend_topk
    ids, sc, st = recommend_topk(np.ones((4, 3), np.float64), np.ones((6, 3), np.float32), k=2, users=np.zeros(0, np.int64))
    assert ids.shape == (0, 2) and ids.dtype == np.int32 and sc.shape == (0, 2) and sc.dtype == np.float64 and st.shape == (0,)


def test_bad_arguments_of_the_c_entry_are_refused_without_a_device():
    """m == 0 is RM_OK and writes nothing; a k_top outside [1, n] and null outputs are RM_ERR_INVALID: decided on the host"""
    import ctypes as C
    from recometrics_amd import _binding
    lib = _binding.load()
    A = np.ones((2, 4), np.float32)
    B = np.ones((8, 4), np.float32)
    idx = np.full((2, 3), 77, np.int32)
    sc = np.full((2, 3), 7.0, np.float32)
    st = np.full(2, 77, np.int32)
    p = _binding._p
    assert lib.rm_recommend_f32(p(A), 4, p(B), 4, 0, 8, 4, None, None, 3, p(idx), p(sc), p(st), 0) == 0
    assert (idx == 77).all() and (sc == 7.0).all() and (st == 77).all()
    for k_top in (0, 9):
        assert lib.rm_recommend_f32(p(A), 4, p(B), 4, 2, 8, 4, None, None, k_top, p(idx), p(sc), p(st), 0) == 1
        assert b"k_top" in lib.rm_last_error()
    assert lib.rm_recommend_f32(p(A), 4, p(B), 4, 2, 8, 4, None, None, 3, None, p(sc), p(st), 0) == 1
    assert lib.rm_recommend_dev_f32(p(A), 4, p(B), 4, 2, 8, 4, None, None, C.c_int64(0), 3, p(idx), p(sc), None, None) == 1
    assert (idx == 77).all() and (st == 77).all()


def test_no_device_is_a_loud_error_not_a_fallback():
    """Without a GPU the call raises, as rank does (tests/test_cabi_exports.py): never a list computed on the CPU"""
    from recometrics_amd import _binding, recommend_topk
    if _binding.device_count() > 0:
        pytest.skip("a GPU is present")
    A = np.ones((2, 4), np.float32)
    B = np.ones((8, 4), np.float32)
    with pytest.raises((RuntimeError, MemoryError)):
        recommend_topk(A, B, k=2)
    with pytest.raises((RuntimeError, MemoryError)):
        _binding.recommend(A, 4, B, 4, np.zeros(3, np.int32), np.zeros(0, np.int32), 2)
