"""CPU-only: the metrics from a caller's score matrix (rm_calc_metrics_scores_* / calc_reco_metrics_from_scores) -- what is decided
without a device: the exports, m == 0, every RM_ERR_INVALID case of the header, "no device is an error, not a fallback", and the
argument errors of the Python function, which raise before the library is touched."""
import ctypes as C

import numpy as np
import pytest

RM_OK, RM_ERR_INVALID, RM_ERR_HIP = 0, 1, 2
SYMBOLS = ("rm_calc_metrics_scores_f32", "rm_calc_metrics_scores_f64", "rm_calc_metrics_scores_dev_f32", "rm_calc_metrics_scores_dev_f64")


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import build as rb
    rb.build()
    from recometrics_amd import _binding
    _binding.load()
    return _binding


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _problem(dtype=np.float32, m=3, n=8):
    S = np.arange(m * n, dtype=dtype).reshape(m, n)
    trp = np.array([0, 1, 2, 3][:m + 1], np.int32)
    tri = np.array([0, 1, 2][:m], np.int32)
    tep = np.array([0, 1, 2, 3][:m + 1], np.int32)
    tei = np.array([5, 6, 7][:m], np.int32)
    tev = np.ones(m, dtype)
    return S, trp, tri, tep, tei, tev


def _host(hip, S, lds, m, n, trp, tri, tep, tei, tev, K, outs=None, dtype=np.float32):
    """the raw host entry: status and message"""
    lib = hip.load()
    fn = getattr(lib, "rm_calc_metrics_scores_" + ("f32" if dtype == np.float32 else "f64"))
    if outs is None:
        outs = [np.empty(max(m, 1), dtype)] + [None] * 9
    rc = fn(_p(S), lds, m, n, _p(trp), _p(tri), _p(tep), _p(tei), _p(tev), K, 0, *[_p(o) for o in outs], 1, 2, 1, 1)
    return rc, (lib.rm_last_error() or b"").decode()


def _dev(hip, S, lds, m, n, trp, tri, tep, tei, tev, K, outs=None, dtype=np.float32):
    """the raw device entry, handed HOST addresses: only good for the checks that come before any device work"""
    lib = hip.load()
    fn = getattr(lib, "rm_calc_metrics_scores_dev_" + ("f32" if dtype == np.float32 else "f64"))
    if outs is None:
        outs = [np.empty(max(m, 1), dtype)] + [None] * 9
    rc = fn(_p(S), lds, m, n, _p(trp), _p(tri), int(tri.shape[0]), _p(tep), _p(tei), _p(tev), int(tei.shape[0]), K, 0,
            *[_p(o) for o in outs], 1, 2, 1, None)
    return rc, (lib.rm_last_error() or b"").decode()


def test_the_four_symbols_are_exported_and_declared(hip):
    lib = hip.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hip.EXPORTS
    assert callable(hip.calc_metrics_scores) and callable(hip.calc_metrics_scores_device)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("entry", [_host, _dev])
def test_no_user_is_ok_and_writes_nothing(hip, dtype, entry):
    S, trp, tri, tep, tei, tev = _problem(dtype)
    out = np.full(4, 7.0, dtype)
    rc, _ = entry(hip, S, 8, 0, 8, trp, tri, tep, tei, tev, 2, outs=[out] + [None] * 9, dtype=dtype)
    assert rc == RM_OK and (out == 7.0).all()
    # (nothing is looked at: not even null pointers)
    rc, _ = entry(hip, None, 0, 0, 0, trp, tri, tep, tei, tev, 0, outs=[out] + [None] * 9, dtype=dtype)
    assert rc == RM_OK and (out == 7.0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("entry", [_host, _dev])
def test_invalid_arguments_are_decided_without_a_device(hip, dtype, entry):
    S, trp, tri, tep, tei, tev = _problem(dtype)
    m, n = S.shape
    cases = {
        "lds < n": dict(lds=n - 1),
        "n <= 0": dict(n=0),
        "n < 0": dict(n=-3),
        "k_metrics = 0": dict(K=0),
        "k_metrics < 0": dict(K=-1),
        "k_metrics > n": dict(K=n + 1),
        "null S": dict(S=None),
        "m < 0": dict(m=-1),
    }
    for what, change in cases.items():
        kw = dict(S=S, lds=n, m=m, n=n, K=2)
        kw.update(change)
        rc, msg = entry(hip, kw["S"], kw["lds"], kw["m"], kw["n"], trp, tri, tep, tei, tev, kw["K"], dtype=dtype)
        assert rc == RM_ERR_INVALID and msg, (what, rc, msg)
    # NDCG requested without test values
    outs = [None] * 10
    outs[5] = np.empty(m, dtype)
    rc, msg = entry(hip, S, n, m, n, trp, tri, tep, tei, None, 2, outs=outs, dtype=dtype)
    assert rc == RM_ERR_INVALID and "NDCG" in msg
    # messages that name what was wrong
    rc, msg = entry(hip, S, n - 1, m, n, trp, tri, tep, tei, tev, 2, dtype=dtype)
    assert "leading dimension" in msg
    rc, msg = entry(hip, S, n, m, n, trp, tri, tep, tei, tev, n + 1, dtype=dtype)
    assert "k_metrics" in msg and str(n) in msg


def test_bad_index_pointers_are_invalid_on_the_host_entry(hip):
    S, trp, tri, tep, tei, tev = _problem()
    bad = tep.copy()
    bad[2] = 0
    rc, msg = _host(hip, S, 8, 3, 8, trp, tri, bad, tei, tev, 2)
    assert rc == RM_ERR_INVALID and "row 1" in msg


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_device_is_an_error_not_a_fallback(hip, dtype):
    if hip.device_count() > 0:
        pytest.skip("a GPU is present")
    S, trp, tri, tep, tei, tev = _problem(dtype)
    out = np.full(3, 7.0, dtype)
    rc, msg = _host(hip, S, 8, 3, 8, trp, tri, tep, tei, tev, 2, outs=[out] + [None] * 9, dtype=dtype)
    assert rc == RM_ERR_HIP and msg and (out == 7.0).all()
    rc, msg = _dev(hip, S, 8, 3, 8, trp, tri, tep, tei, tev, 2, outs=[out] + [None] * 9, dtype=dtype)
    assert rc == RM_ERR_HIP and msg and (out == 7.0).all()
    want = {name: name == "p" for name in hip.METRIC_ORDER}
    with pytest.raises(RuntimeError):
        hip.calc_metrics_scores(S, 8, trp, tri, tep, tei, tev, 2, want, False, True, 2, 1, 1)


# ---- the Python function: every argument error raises before the library is touched ---------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    """any call into the binding fails the test"""
    from recometrics_amd import _binding

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    for name in ("load", "calc_metrics_scores", "calc_metrics", "has_openmp"):
        monkeypatch.setattr(_binding, name, boom)


def _py_problem(dtype=np.float64, m=4, n=9):
    from scipy.sparse import csr_array
    rng = np.random.default_rng(0)
    S = rng.standard_normal((m, n)).astype(dtype)
    X_train = csr_array((np.ones(m), (np.arange(m), np.arange(m))), shape=(m, n))
    X_test = csr_array((np.ones(m), (np.arange(m), np.arange(m) + 3)), shape=(m, n))
    return X_train, X_test, S


def test_the_function_is_exported():
    import recometrics_amd
    assert "calc_reco_metrics_from_scores" in recometrics_amd.__all__
    assert callable(recometrics_amd.calc_reco_metrics_from_scores)
    import inspect
    params = inspect.signature(recometrics_amd.calc_reco_metrics_from_scores).parameters
    ref = inspect.signature(recometrics_amd.calc_reco_metrics).parameters
    for gone in ("break_ties_with_noise", "seed", "item_biases", "A", "B"):
        assert gone not in params
    for name in params:
        if name != "scores":
            assert name in ref and params[name].default == ref[name].default, name
    doc = recometrics_amd.calc_reco_metrics_from_scores.__doc__
    assert "break_ties_with_noise" in doc and "seed" in doc and "item_biases" in doc


def test_python_argument_errors(no_library):
    from recometrics_amd import calc_reco_metrics_from_scores as f
    X_train, X_test, S = _py_problem()
    m, n = S.shape
    with pytest.raises(ValueError, match="same shape"):
        f(X_train, X_test, S[:, :-1])
    with pytest.raises(ValueError, match="same shape"):
        f(X_train, X_test, S[:-1])
    with pytest.raises(ValueError, match="same shape"):
        f(X_train, X_test, np.ascontiguousarray(S.T))
    with pytest.raises(ValueError, match="2-dimensional"):
        f(X_train, X_test, S.reshape(-1))
    with pytest.raises(ValueError, match="NumPy array"):
        f(X_train, X_test, S.tolist())
    with pytest.raises(ValueError, match="numeric"):
        f(X_train, X_test, S.astype(str))
    with pytest.raises(ValueError, match="'k' should be smaller than the number of items."):
        f(X_train, X_test, S, k=n + 1)
    with pytest.raises(ValueError, match="'k' must be positive"):
        f(X_train, X_test, S, k=0)
    with pytest.raises(ValueError, match="at least one metric"):
        f(X_train, X_test, S, precision=False, average_precision=False, ndcg=False)
    with pytest.raises(ValueError, match="'X_test' is empty."):
        f(X_train, type(X_test)(X_test.shape), S)
    with pytest.raises(ValueError, match="same number of rows"):
        f(X_train[:-1], X_test, S)
    with pytest.raises(ValueError, match="same number of columns"):
        f(X_train[:, :-1], X_test, S)
    with pytest.raises(ValueError, match="sparse"):
        f(X_train, X_test.toarray(), S)
    with pytest.raises(ValueError, match="sparse"):
        f(X_train.toarray(), X_test, S)
    with pytest.raises(ValueError, match="min_pos_test"):
        f(X_train, X_test, S, min_pos_test=0)
    with pytest.raises(ValueError, match="nthreads"):
        f(X_train, X_test, S, nthreads=0)
    with pytest.raises(TypeError):
        f(X_train, X_test, S, break_ties_with_noise=False)
    with pytest.raises(TypeError):
        f(X_train, X_test, S, seed=1)


def test_scores_reach_the_binding_as_they_are(monkeypatch):
    """float32 only when float32, otherwise float64; a row-major array -- dense or with a row stride -- is not copied, a
    Fortran-ordered one is copied once; X_train=None is an empty matrix with consider_cold_start=True"""
    from recometrics_amd import _binding, calc_reco_metrics_from_scores as f
    seen = {}

    def fake(S, lds, trp, tri, tep, tei, tev, k, want, cumulative, cold, mip, mpt, nthreads, outs=None):
        seen.update(S=S, lds=lds, trp=trp, tri=tri, tev=tev, cold=cold, k=k, want=want, outs=outs)
        for o in outs or []:
            o[...] = 0.5
        return tuple(outs) if outs is not None else tuple(np.zeros(S.shape[0] if want[nm] else 0, S.dtype) for nm in _binding.METRIC_ORDER)
    monkeypatch.setattr(_binding, "calc_metrics_scores", fake)
    X_train, X_test, S = _py_problem(np.float32)
    m, n = S.shape
    df = f(X_train, X_test, S, k=3)
    assert seen["S"] is S and seen["lds"] == n and seen["S"].dtype == np.float32 and seen["tev"].dtype == np.float32
    assert list(df.columns) == ["P@3", "AP@3", "NDCG@3"] and df.shape == (m, 3) and (df.values == 0.5).all()
    wide = np.zeros((m, n + 5), np.float32)
    view = wide[:, 2:2 + n]
    f(X_train, X_test, view, k=3)
    assert seen["S"] is view and seen["lds"] == n + 5
    fort = np.asfortranarray(S)
    f(X_train, X_test, fort, k=3)
    assert seen["S"] is not fort and seen["S"].flags["C_CONTIGUOUS"] and seen["lds"] == n and (seen["S"] == S).all()
    for other in (np.float64, np.float16, np.int32):
        f(X_train, X_test, S.astype(other), k=3)
        assert seen["S"].dtype == np.float64 and seen["tev"].dtype == np.float64
    f(None, X_test, S, k=3, consider_cold_start=False)
    assert seen["cold"] is True and seen["trp"].shape == (m + 1,) and not seen["trp"].any() and seen["tri"].shape == (0,)
    out = f(X_train, X_test, S, k=3, as_df=False, all_metrics=True)
    assert out["K"] == 3 and all(seen["want"].values())
