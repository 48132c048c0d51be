"""CPU-only: the recommendation lists from a caller's score matrix (rm_recommend_scores_* / recommend_topk_from_scores) -- what is
decided without a device: the declarations and exports, m == 0, every RM_ERR_INVALID case of the header, "no device is an error, not
a fallback", the argument errors of the Python function (raised before the library is touched) and what reaches the binding.
(What the lists hold is tests/test_hip_recommend_scores.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_OK, RM_ERR_INVALID, RM_ERR_HIP = 0, 1, 2
SYMBOLS = ("rm_recommend_scores_f32", "rm_recommend_scores_f64", "rm_recommend_scores_dev_f32", "rm_recommend_scores_dev_f64")


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import build as rb
    rb.build()
    from recometrics_amd import _binding
    _binding.load()
    return _binding


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _outputs(dtype, m=3, K=2):
    return np.full((max(m, 1), K), 77, np.int32), np.full((max(m, 1), K), 7.0, dtype), np.full(max(m, 1), 77, np.int32)


def _host(hip, S, lds, m, n, K, idx, sc, st, dtype=np.float32, xp=None, xi=None):
    """the raw host entry: status and message"""
    lib = hip.load()
    fn = getattr(lib, "rm_recommend_scores_" + ("f32" if dtype == np.float32 else "f64"))
    rc = fn(_p(S), lds, m, n, _p(xp), _p(xi), K, _p(idx), _p(sc), _p(st), 1)
    return rc, (lib.rm_last_error() or b"").decode()


def _dev(hip, S, lds, m, n, K, idx, sc, st, dtype=np.float32, xp=None, xi=None, nnz=0):
    """the raw device entry, handed HOST addresses: only good for the checks that come before any device work"""
    lib = hip.load()
    fn = getattr(lib, "rm_recommend_scores_dev_" + ("f32" if dtype == np.float32 else "f64"))
    rc = fn(_p(S), lds, m, n, _p(xp), _p(xi), C.c_int64(nnz), K, _p(idx), _p(sc), _p(st), None)
    return rc, (lib.rm_last_error() or b"").decode()


def test_header_declares_the_four_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "recometrics_hip.h")).read(), flags=re.S)
    for sym in SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % sym, text)
        assert decl, "not declared: " + sym
        args = decl.group(1)
        real = "float" if sym.endswith("f32") else "double"
        for piece in ("const %s *S" % real, "size_t lds", "Xexcl_csr_p", "Xexcl_csr_i", "int32_t k_top", "int32_t *idx", real + " *score",
                      "int32_t *status"):
            assert piece in args, (sym, piece)
        assert ("int64_t nnz_excl" in args and "void *stream" in args) == ("_dev_" in sym), sym
        assert ("int32_t nthreads" in args) == ("_dev_" not in sym), sym


def test_the_four_symbols_are_exported_and_bound(hip):
    lib = hip.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hip.EXPORTS
    assert callable(hip.recommend_scores) and callable(hip.recommend_scores_device)


def test_public_function_is_exported():
    import recometrics_amd
    assert "recommend_topk_from_scores" in recometrics_amd.__all__
    assert callable(recometrics_amd.recommend_topk_from_scores)
    assert {"calc_reco_metrics", "calc_reco_metrics_from_scores", "recommend_topk", "split_reco_train_test"} <= set(recometrics_amd.__all__)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("entry", [_host, _dev])
def test_no_user_is_ok_and_writes_nothing(hip, dtype, entry):
    S = np.arange(24, dtype=dtype).reshape(3, 8)
    idx, sc, st = _outputs(dtype)
    rc, _ = entry(hip, S, 8, 0, 8, 2, idx, sc, st, dtype=dtype)
    assert rc == RM_OK and (idx == 77).all() and (sc == 7.0).all() and (st == 77).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("entry", [_host, _dev])
def test_invalid_arguments_are_decided_without_a_device(hip, dtype, entry):
    S = np.arange(24, dtype=dtype).reshape(3, 8)
    m, n = S.shape
    idx, sc, st = _outputs(dtype)
    cases = {
        "null S": dict(S=None),
        "lds < n": dict(lds=n - 1),
        "n <= 0": dict(n=0),
        "n < 0": dict(n=-3),
        "m < 0": dict(m=-1),
        "k_top = 0": dict(K=0),
        "k_top = n + 1": dict(K=n + 1),
        "null idx": dict(idx=None),
        "null status": dict(st=None),
    }
    for what, change in cases.items():
        kw = dict(S=S, lds=n, m=m, n=n, K=2, idx=idx, st=st)
        kw.update(change)
        rc, msg = entry(hip, kw["S"], kw["lds"], kw["m"], kw["n"], kw["K"], kw["idx"], sc, kw["st"], dtype=dtype)
        assert rc == RM_ERR_INVALID and msg, (what, rc, msg)
        assert (idx == 77).all() and (sc == 7.0).all() and (st == 77).all(), what
    rc, msg = entry(hip, S, n - 1, m, n, 2, idx, sc, st, dtype=dtype)
    assert "leading dimension" in msg
    rc, msg = entry(hip, S, n, m, n, n + 1, idx, sc, st, dtype=dtype)
    assert "k_top" in msg and str(n) in msg


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_negative_length_of_the_index_array_is_invalid(hip, dtype):
    S = np.arange(24, dtype=dtype).reshape(3, 8)
    idx, sc, st = _outputs(dtype)
    xp, xi = np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)
    rc, msg = _dev(hip, S, 8, 3, 8, 2, idx, sc, st, dtype=dtype, xp=xp, xi=xi, nnz=-1)
    assert rc == RM_ERR_INVALID and msg and (idx == 77).all() and (st == 77).all()


def test_bad_index_pointers_are_invalid_on_the_host_entry(hip):
    S = np.arange(24, dtype=np.float32).reshape(3, 8)
    idx, sc, st = _outputs(np.float32)
    xp, xi = np.array([0, 2, 1, 3], np.int32), np.array([0, 1, 2], np.int32)
    rc, msg = _host(hip, S, 8, 3, 8, 2, idx, sc, st, xp=xp, xi=xi)
    assert rc == RM_ERR_INVALID and "row 1" in msg


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_device_is_an_error_not_a_fallback(hip, dtype):
    if hip.device_count() > 0:
        pytest.skip("a GPU is present")
    from recometrics_amd import recommend_topk_from_scores
    S = np.arange(24, dtype=dtype).reshape(3, 8)
    idx, sc, st = _outputs(dtype)
    for entry in (_host, _dev):
        rc, msg = entry(hip, S, 8, 3, 8, 2, idx, sc, st, dtype=dtype)
        assert rc == RM_ERR_HIP and msg and (idx == 77).all() and (sc == 7.0).all() and (st == 77).all()
    with pytest.raises(RuntimeError):
        hip.recommend_scores(S, 8, None, None, 2)
    with pytest.raises(RuntimeError):
        recommend_topk_from_scores(S, k=2)


# ---- the Python function ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    """any call into the binding fails the test"""
    from recometrics_amd import _binding

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    for name in ("load", "recommend_scores", "recommend", "calc_metrics_scores"):
        monkeypatch.setattr(_binding, name, boom)


def test_python_argument_errors(no_library):
    from scipy.sparse import csr_array
    from recometrics_amd import recommend_topk_from_scores as f
    S = np.random.default_rng(0).standard_normal((4, 9))
    m, n = S.shape
    X = csr_array((np.ones(m), (np.arange(m), np.arange(m))), shape=(m, n))
    with pytest.raises(ValueError, match="NumPy array"):
        f(S.tolist())
    with pytest.raises(ValueError, match="2-dimensional"):
        f(S.reshape(-1), k=2)
    with pytest.raises(ValueError, match="numeric"):
        f(S.astype(str), k=2)
    with pytest.raises(ValueError, match="'k' must be positive"):
        f(S, k=0)
    with pytest.raises(ValueError, match="'k' should be smaller than the number of items."):
        f(S, k=n + 1)
    with pytest.raises(ValueError, match="sparse"):
        f(S, k=2, X_train=X.toarray())
    with pytest.raises(ValueError, match="same shape"):
        f(S, k=2, X_train=X[:-1])
    with pytest.raises(ValueError, match="same shape"):
        f(S, k=2, X_train=X[:, :-1])
    for bad in ([0, m], [-1], [1.5], [[0, 1]]):
        with pytest.raises(ValueError, match="'users'"):
            f(S, k=2, users=np.array(bad))


def test_no_users_asked_for_is_an_empty_answer(no_library):
    from recometrics_amd import recommend_topk_from_scores as f
    ids, sc, st = f(np.ones((4, 6), np.float32), k=2, users=[])
    assert ids.shape == (0, 2) and ids.dtype == np.int32 and sc.shape == (0, 2) and sc.dtype == np.float32 and st.shape == (0,)
    ids, sc, st = f(np.ones((0, 6), np.int64), k=2, return_scores=False)
    assert ids.shape == (0, 2) and sc is None and st.shape == (0,) and st.dtype == np.int32


def test_scores_reach_the_binding_as_they_are(monkeypatch):
    """float32 only when float32, otherwise float64; a row-major array -- dense or with a row stride -- is not copied, a
    Fortran-ordered one is copied once; `users=` gathers rows of the scores and of X_train once, in that order; X_train is untouched"""
    from scipy.sparse import coo_array, csr_array
    from recometrics_amd import _binding, recommend_topk_from_scores as f
    seen = {}

    def fake(S, lds, excl_p, excl_i, k_top, return_scores=True, nthreads=0):
        seen.update(S=S, lds=lds, excl_p=excl_p, excl_i=excl_i, k=k_top, rs=return_scores)
        return "ids", "scores", "status"
    monkeypatch.setattr(_binding, "recommend_scores", fake)
    S = np.random.default_rng(1).standard_normal((4, 9)).astype(np.float32)
    m, n = S.shape
    assert f(S, k=3) == ("ids", "scores", "status")
    assert seen["S"] is S and seen["lds"] == n and seen["excl_p"] is None and seen["excl_i"] is None and seen["k"] == 3 and seen["rs"] is True
    wide = np.zeros((m, n + 5), np.float32)
    view = wide[:, 2:2 + n]
    f(view, k=3, return_scores=False)
    assert seen["S"] is view and seen["lds"] == n + 5 and seen["S"].ctypes.data == wide.ctypes.data + 8 and seen["rs"] is False
    fort = np.asfortranarray(S)
    f(fort, k=3)
    assert seen["S"] is not fort and seen["S"].flags["C_CONTIGUOUS"] and seen["lds"] == n and (seen["S"] == S).all()
    for other in (np.float64, np.float16, np.int32, np.uint8, bool):
        f(S.astype(other), k=3)
        assert seen["S"].dtype == np.float64 and (seen["S"] == S.astype(other).astype(np.float64)).all()
    rows = np.array([0, 0, 1, 2, 3, 3]), np.array([1, 5, 0, 8, 2, 4])
    X64 = csr_array((np.ones(6), rows), shape=(m, n))
    X64 = csr_array((X64.data, X64.indices.astype(np.int64), X64.indptr.astype(np.int64)), shape=(m, n))
    f(S, k=3, X_train=X64)
    assert seen["excl_p"].dtype == np.int32 and seen["excl_p"].tolist() == [0, 2, 3, 4, 6] and seen["excl_i"].dtype == np.int32
    assert seen["excl_i"].tolist() == [1, 5, 0, 8, 2, 4] and X64.indices.dtype == np.int64
    f(S, k=3, X_train=coo_array(X64), users=np.array([3, 0]))
    assert (seen["S"] == S[[3, 0]]).all() and seen["lds"] == n and seen["excl_p"].tolist() == [0, 2, 4] and seen["excl_i"].tolist() == [2, 4, 1, 5]
