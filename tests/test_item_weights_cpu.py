"""CPU-only: item-item models (include/recometrics_hip_item_weights.h, calc_reco_metrics_from_item_weights,
recommend_topk_from_item_weights) -- what is decided without a device: the header against _binding.ITEM_WEIGHT_SIGNATURES, the exports,
m == 0, every host-decided RM_ERR_INVALID with its message and the outputs untouched, and the public functions' ValueErrors.  (What the
entries compute is tests/test_hip_item_weights.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_factors_half_cpu import _p, hip  # noqa: F401 (hip: a fixture -- the library, built)
from test_scores_half_cpu import _c_kind, _ctypes_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_OK, RM_ERR_INVALID = 0, 1
SYMBOLS = tuple("rm_%s_item_weights%s_%s" % (request, form, suffix) for request in ("calc_metrics", "recommend") for form in ("", "_dev")
                for suffix in ("f32", "f64"))
M, N, N_IN = 3, 8, 5


def test_the_binding_states_every_declaration_of_the_header():
    from recometrics_amd import _binding
    text = open(os.path.join(ROOT, "include", "recometrics_hip_item_weights.h")).read()
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    declared = re.findall(r"([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*;", text)
    table = _binding.ITEM_WEIGHT_SIGNATURES
    assert [name for _, name, _ in declared] == list(SYMBOLS) and set(table) == set(SYMBOLS)
    for other in (_binding.SIGNATURES, _binding.HALF_SIGNATURES, _binding.HALF_FACTOR_SIGNATURES, _binding.CAND_SIGNATURES, _binding.CAND_METRIC_SIGNATURES):
        assert not set(table) & set(other)
    for ret, name, params in declared:
        params = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        mine, restype = table[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(" ".join(t.split())) for t, _ in params], name
        assert ret.strip() == "int" and _ctypes_kind(restype) == ("signed", 4), name
        assert [n for _, n in params][:8] == ["W", "ldw", "n_in", "m", "n", "hist_p", "hist_i", "hist_v"], name
        real = "double" if name.endswith("f64") else "float"
        assert [" ".join(t.split()) for t, n in params if n in ("W", "hist_v")] == ["const %s *" % real] * 2, name


def test_the_library_exports_all_eight(hip):
    import recometrics_amd
    lib = hip.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), "missing export: " + sym
        assert getattr(lib, sym).argtypes == [t for _, t in hip.ITEM_WEIGHT_SIGNATURES[sym][0]]
    assert {"calc_reco_metrics_from_item_weights", "recommend_topk_from_item_weights"} <= set(recometrics_amd.__all__)


def _call(hip, request, dtype, dev, **change):
    """(status, message, outputs untouched) of an entry on a small valid request with `change` applied; the outputs start as 77 / 7.0"""
    kw = dict(W=np.ones((N_IN, N), dtype), ldw=N, n_in=N_IN, m=M, n=N, hp=np.array([0, 1, 2, 3], np.int32), hi=np.array([0, 1, 2], np.int32),
              hv=np.ones(3, dtype), nnz_hist=3, xp=np.array([0, 1, 2, 3], np.int32), xi=np.array([3, 4, 5], np.int32), nnz=3,
              tp=np.array([0, 1, 2, 3], np.int32), ti=np.array([0, 1, 2], np.int32), tv=np.ones(3, dtype), nnz_test=3, K=2,
              p=np.full(M, 7.0, dtype), ndcg=np.full(M, 7.0, dtype), idx=np.full((M, 2), 77, np.int32), st=np.full(M, 77, np.int32))
    kw.update(change)
    lib = hip.load()
    fn = getattr(lib, "rm_%s_item_weights_%s%s" % (request, "dev_" if dev else "", "f32" if dtype == np.float32 else "f64"))
    length = lambda name: (C.c_int64(kw[name]),) if dev else ()
    head = (_p(kw["W"]), kw["ldw"], kw["n_in"], kw["m"], kw["n"], _p(kw["hp"]), _p(kw["hi"]), _p(kw["hv"]), *length("nnz_hist"),
            _p(kw["xp"]), _p(kw["xi"]), *length("nnz"))
    if request == "recommend":
        rc = fn(*head, kw["K"], _p(kw["idx"]), None, _p(kw["st"]), None if dev else 1)
        outs = ("idx", "st")
    else:
        rc = fn(*head, _p(kw["tp"]), _p(kw["ti"]), _p(kw["tv"]), *length("nnz_test"), kw["K"], 0,
                _p(kw["p"]), None, None, None, None, _p(kw["ndcg"]), None, None, None, None, 1, 2, 1, None if dev else 1)
        outs = ("p", "ndcg")
    untouched = all((kw[name] == (77 if name in ("idx", "st") else 7.0)).all() for name in outs if kw[name] is not None)
    return rc, (lib.rm_last_error() or b"").decode(), untouched


SHARED = {"null W": (dict(W=None), "null input pointer"), "null hist_p": (dict(hp=None), "null input pointer"),
          "n <= 0": (dict(n=0), "n and n_in must be positive"), "n_in <= 0": (dict(n_in=0), "n and n_in must be positive"),
          "m < 0": (dict(m=-1), "m must not be negative"), "ldw < n": (dict(ldw=N - 1), "leading dimension of the weight matrix smaller than n"),
          "k < 1": (dict(K=0), r"must lie in \[1, n\]"), "k > n": (dict(K=N + 1), r"must lie in \[1, n\]")}
ONLY = {"calc_metrics": {"null Xtrain_csr_p": (dict(xp=None), "null input pointer"), "null Xtest_csr_p": (dict(tp=None), "null input pointer"),
                         "null Xtest_csr_i": (dict(ti=None), "null input pointer"), "NDCG without test values": (dict(tv=None), "NDCG requested without test values")},
        "recommend": {"null idx": (dict(idx=None), "null output pointer"), "null status": (dict(st=None), "null output pointer")}}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("request_", ["calc_metrics", "recommend"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_what_the_host_decides(hip, dtype, request_, dev):
    descending = np.array([0, 2, 1, 3], np.int32)
    form = (dict({"nnz_hist < 0": (dict(nnz_hist=-1), "negative length"), "null hist_i": (dict(hi=None), "null input pointer"),
                  "nnz_train / nnz_excl < 0": (dict(nnz=-1), "negative length"), "null train / excl indices": (dict(xi=None), "null input pointer")},
                 **({"nnz_test < 0": (dict(nnz_test=-1), "negative length")} if request_ == "calc_metrics" else {})) if dev else
            {"descending history pointers": (dict(hp=descending), r"row 1 are negative or decreasing \(X_hist\)"),
             "descending pointers": (dict(xp=descending), "row 1 are negative or decreasing"), "null hist_i": (dict(hi=None), "null history indices")})
    for what, (change, message) in dict(SHARED, **ONLY[request_], **form).items():
        rc, msg, untouched = _call(hip, request_, dtype, dev, **change)
        assert rc == RM_ERR_INVALID and re.search(message, msg) and untouched, (what, rc, msg)
    assert _call(hip, request_, dtype, dev, m=0)[::2] == (RM_OK, True)
    if hip.device_count() == 0:                                       # without a device the call is an error, never a computation on the CPU
        rc, msg, untouched = _call(hip, request_, dtype, dev)
        assert rc not in (RM_OK, RM_ERR_INVALID) and msg and untouched


def test_the_public_functions_before_they_reach_the_library(monkeypatch):
    import torch
    from scipy.sparse import csr_array
    from recometrics_amd import _binding, calc_reco_metrics_from_item_weights as calc, recommend_topk_from_item_weights as reco
    W = np.ones((N_IN, N), np.float32)
    X_hist = csr_array((np.ones(3, np.float32), np.array([0, 1, 2], np.int32), np.array([0, 1, 2, 3], np.int32)), shape=(M, N_IN))
    X_train = csr_array((np.ones(3, np.float32), np.array([3, 4, 5], np.int32), np.array([0, 1, 2, 3], np.int32)), shape=(M, N))
    X_test = csr_array((np.ones(3, np.float32), np.array([0, 1, 2], np.int32), np.array([0, 1, 2, 3], np.int32)), shape=(M, N))

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    for name in ("load", "calc_metrics_item_weights", "calc_metrics_item_weights_device", "recommend_item_weights", "recommend_item_weights_device"):
        monkeypatch.setattr(_binding, name, reached)
    half = [torch.ones((N_IN, N), dtype=t) for t in (torch.float16, torch.bfloat16)] + [W.astype(np.float16)]
    for bad, message in ([(dict(W=h), "16-bit 'W' is not supported") for h in half] + [
            (dict(W=W[:, :N - 1]), "columns of 'W' and of 'X_test'"), (dict(W=W[:N_IN - 1]), "columns of 'X_hist' and of rows of 'W'"),
            (dict(X_hist=None), "columns of 'X_hist' and of rows of 'W'"),         # (X_train in its place: N columns against N_IN rows)
            (dict(X_hist=None, X_train=None), "'X_hist' must be passed"), (dict(X_hist=X_hist[:2]), "same number of rows"),
            (dict(k=0), "'k' must be positive"), (dict(k=N + 1), "'k' should be smaller"), (dict(W=np.ones(N)), "2-dimensional"),
            (dict(precision=False, average_precision=False, ndcg=False), "at least one metric")]):
        with pytest.raises(ValueError, match=message):
            calc(**dict(dict(X_train=X_train, X_test=X_test, W=W, X_hist=X_hist), **bad))
    for bad, message in ([(dict(W=h), "16-bit 'W' is not supported") for h in half] + [
            (dict(W=W[:N_IN - 1]), "columns of 'X_hist' and of rows of 'W'"), (dict(k=0), "'k' must be positive"), (dict(k=N + 1), "'k' should be smaller"),
            (dict(X_train=X_train[:2]), "'X_train' must have a row per user"), (dict(users=[M]), "'users' has entries outside")]):
        with pytest.raises(ValueError, match=message):
            reco(**dict(dict(X_hist=X_hist, W=W, k=2), **bad))
    with pytest.raises(AssertionError, match="the library was reached"):
        reco(X_hist, W, k=2)
