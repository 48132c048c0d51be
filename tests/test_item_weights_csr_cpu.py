"""CPU-only: item-item models with a sparse W (include/recometrics_hip_item_weights_csr.h) -- what is decided without a device, as
tests/test_item_weights_cpu.py does it for the dense entries.  (What the entries compute is tests/test_hip_item_weights_csr.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_factors_half_cpu import _p, hip  # noqa: F401 (hip: a fixture -- the library, built)
from test_item_weights_cpu import M, N, N_IN, ONLY, RM_ERR_INVALID, RM_OK, ROOT
from test_item_weights_cpu import SHARED as DENSE_SHARED
from test_scores_half_cpu import _c_kind, _ctypes_kind

SYMBOLS = tuple("rm_%s_item_weights_csr%s_%s" % (request, form, suffix) for request in ("calc_metrics", "recommend") for form in ("", "_dev")
                for suffix in ("f32", "f64"))


def test_the_binding_states_every_declaration_of_the_header_and_the_library_exports_them(hip):
    from recometrics_amd import _binding
    text = open(os.path.join(ROOT, "include", "recometrics_hip_item_weights_csr.h")).read()
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    declared = re.findall(r"([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*;", text)
    table = _binding.ITEM_WEIGHT_CSR_SIGNATURES
    assert [name for _, name, _ in declared] == list(SYMBOLS) and set(table) == set(SYMBOLS)
    for other in (_binding.SIGNATURES, _binding.HALF_SIGNATURES, _binding.HALF_FACTOR_SIGNATURES, _binding.CAND_SIGNATURES,
                  _binding.CAND_METRIC_SIGNATURES, _binding.ITEM_WEIGHT_SIGNATURES, _binding.TEST_HOOKS):
        assert not set(table) & set(other)
    for ret, name, params in declared:
        params = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        mine, restype = table[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(" ".join(t.split())) for t, _ in params], name
        assert ret.strip() == "int" and _ctypes_kind(restype) == ("signed", 4), name
        assert [n for _, n in params][:9] == ["W_p", "W_i", "W_v", "n_in", "m", "n", "hist_p", "hist_i", "hist_v"], name
        assert ([n for _, n in params][9:11] == ["nnz_hist", "nnz_W"]) == ("_dev_" in name), name
        real = "double" if name.endswith("f64") else "float"
        assert [" ".join(t.split()) for t, n in params if n in ("W_v", "hist_v")] == ["const %s *" % real] * 2, name
        assert getattr(hip.load(), name).argtypes == [t for _, t in mine], name


def _call(hip, request, dtype, dev, **change):
    p3, i3 = np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)
    kw = dict(wp=np.arange(N_IN + 1, dtype=np.int32), wi=np.arange(N_IN, dtype=np.int32), wv=np.ones(N_IN, dtype), nnz_W=N_IN, n_in=N_IN, m=M, n=N,
              hp=p3, hi=i3, hv=np.ones(3, dtype), nnz_hist=3, xp=p3, xi=i3 + 3, nnz=3, tp=p3, ti=i3, tv=np.ones(3, dtype), nnz_test=3, K=2,
              p=np.full(M, 7.0, dtype), ndcg=np.full(M, 7.0, dtype), idx=np.full((M, 2), 77, np.int32), st=np.full(M, 77, np.int32))
    kw.update(change)
    lib = hip.load()
    fn = getattr(lib, "rm_%s_item_weights_csr_%s%s" % (request, "dev_" if dev else "", "f32" if dtype == np.float32 else "f64"))
    length = lambda *names: tuple(C.c_int64(kw[name]) for name in names) if dev else ()
    head = (_p(kw["wp"]), _p(kw["wi"]), _p(kw["wv"]), kw["n_in"], kw["m"], kw["n"], _p(kw["hp"]), _p(kw["hi"]), _p(kw["hv"]),
            *length("nnz_hist", "nnz_W"), _p(kw["xp"]), _p(kw["xi"]), *length("nnz"))
    outs = ("idx", "st") if request == "recommend" else ("p", "ndcg")
    if request == "recommend":
        rc = fn(*head, kw["K"], _p(kw["idx"]), None, _p(kw["st"]), None if dev else 1)
    else:
        rc = fn(*head, _p(kw["tp"]), _p(kw["ti"]), _p(kw["tv"]), *length("nnz_test"), kw["K"], 0,
                _p(kw["p"]), None, None, None, None, _p(kw["ndcg"]), None, None, None, None, 1, 2, 1, None if dev else 1)
    untouched = all((kw[name] == (77 if name in ("idx", "st") else 7.0)).all() for name in outs if kw[name] is not None)
    return rc, (lib.rm_last_error() or b"").decode(), untouched


SHARED = dict({what: case for what, case in DENSE_SHARED.items() if what not in ("null W", "ldw < n")},
              **{"null W_p": (dict(wp=None), "null input pointer"), "null W_v": (dict(wv=None), "null input pointer")})


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("request_", ["calc_metrics", "recommend"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_what_the_host_decides(hip, dtype, request_, dev):
    descending = np.array([0, 2, 1, 3], np.int32)
    form = (dict({"nnz_W < 0": (dict(nnz_W=-1), "negative length"), "null W_i": (dict(wi=None), "null input pointer"),
                  "nnz_hist < 0": (dict(nnz_hist=-1), "negative length"), "null hist_i": (dict(hi=None), "null input pointer"),
                  "nnz_train / nnz_excl < 0": (dict(nnz=-1), "negative length"), "null train / excl indices": (dict(xi=None), "null input pointer")},
                 **({"nnz_test < 0": (dict(nnz_test=-1), "negative length")} if request_ == "calc_metrics" else {})) if dev else
            {"descending pointers of W": (dict(wp=np.array([0, 1, 3, 2, 4, 5], np.int32)), r"row 2 are negative or decreasing \(W\)"),
             "null W_i": (dict(wi=None), "null weight indices"),
             "descending history pointers": (dict(hp=descending), r"row 1 are negative or decreasing \(X_hist\)"),
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
    from scipy.sparse import coo_array, csr_array
    from recometrics_amd import _binding, calc_reco_metrics_from_item_weights as calc, recommend_topk_from_item_weights as reco
    W, eye = csr_array(np.eye(N_IN, N, dtype=np.float32)), csr_array(np.eye(M, N, dtype=np.float32))
    X_hist, X_train, X_test = eye[:, :N_IN], eye[:, ::-1], eye

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    for name in ["load"] + [r + "_item_weights_csr" + f for r in ("calc_metrics", "recommend") for f in ("", "_device")]:
        monkeypatch.setattr(_binding, name, reached)
    half16 = csr_array(W)
    half16.data = half16.data.astype(np.float16)                      # (SciPy's constructors refuse the type; the attribute takes it)
    bad_W = ([(h, "16-bit 'W' is not supported") for h in [torch.eye(N_IN, N, dtype=t).to_sparse_csr() for t in (torch.float16, torch.bfloat16)] + [half16]]
             + [(W[:N_IN - 1], "columns of 'X_hist' and of rows of 'W'"), (torch.eye(N_IN, N).to_sparse_coo(), "sparse-CSR layout")])
    for bad, message in bad_W + [(W[:, :N - 1], "columns of 'W' and of 'X_test'")]:
        with pytest.raises(ValueError, match=message):
            calc(X_train, X_test, bad, k=2, X_hist=X_hist)
    for bad, message in bad_W:
        with pytest.raises(ValueError, match=message):
            reco(X_hist, bad, k=2)
    for sparse in (W, coo_array(W), torch.eye(N_IN, N).to_sparse_csr()):      # a valid sparse W does reach the library, in any format
        for call in (lambda: reco(X_hist, sparse, k=2), lambda: calc(X_train, X_test, sparse, k=2, X_hist=X_hist)):
            with pytest.raises(AssertionError, match="the library was reached"):
                call()
