"""CPU-only: metrics over candidate sets (include/recometrics_hip_candidate_metrics.h, calc_reco_metrics_from_candidates) -- what is
decided without a device: the header against _binding.CAND_METRIC_SIGNATURES, the exports, m == 0, every host-decided RM_ERR_INVALID /
RM_ERR_UNSUPPORTED with the outputs untouched, and the public function's ValueErrors.  (What the entries compute is
tests/test_hip_candidate_metrics.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_factors_half_cpu import _p, hip  # noqa: F401 (hip: a fixture -- the library, built)
from test_scores_half_cpu import _c_kind, _ctypes_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_OK, RM_ERR_INVALID, RM_ERR_UNSUPPORTED = 0, 1, 4
SYMBOLS = tuple("rm_calc_metrics_candidates%s_%s" % (form, suffix) for form in ("", "_dev") for suffix in ("f32", "f64"))
M, N, KF = 3, 8, 4


def test_the_binding_states_every_declaration_of_the_header():
    from recometrics_amd import _binding
    text = open(os.path.join(ROOT, "include", "recometrics_hip_candidate_metrics.h")).read()
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    declared = re.findall(r"([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*;", text)
    table = _binding.CAND_METRIC_SIGNATURES
    assert [name for _, name, _ in declared] == list(SYMBOLS) and set(table) == set(SYMBOLS)
    assert not set(table) & (set(_binding.SIGNATURES) | set(_binding.CAND_SIGNATURES))
    for ret, name, params in declared:
        params = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        mine, restype = table[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(" ".join(t.split())) for t, _ in params], name
        assert ret.strip() == "int" and _ctypes_kind(restype) == ("signed", 4), name
        assert not {"break_ties_with_noise", "seed", "consider_cold_start"} & {n for _, n in params}, name
        real = "double" if name.endswith("f64") else "float"
        assert [" ".join(t.split()) for t, n in params if n in ("A", "B", "Xtest_csr", "pr_auc")] == ["const %s *" % real] * 3 + [real + " *"], name


def test_the_library_exports_all_four(hip):
    import recometrics_amd
    lib = hip.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), "missing export: " + sym
        assert getattr(lib, sym).argtypes == [t for _, t in hip.CAND_METRIC_SIGNATURES[sym][0]]
    assert callable(hip.calc_metrics_candidates) and callable(hip.calc_metrics_candidates_device)
    assert "calc_reco_metrics_from_candidates" in recometrics_amd.__all__


def _call(hip, dtype, dev, **change):
    """(status, message, outputs untouched) of an entry on a small valid request with `change` applied; the outputs start as 7.0"""
    kw = dict(A=np.ones((M, KF), dtype), B=np.ones((N, KF), dtype), lda=KF, ldb=KF, m=M, n=N, k=KF, cp=np.array([0, 2, 4, 6], np.int32),
              ci=np.array([0, 1, 1, 2, 2, 3], np.int32), nnz=6, tp=np.array([0, 1, 2, 3], np.int32), ti=np.array([0, 1, 2], np.int32),
              tv=np.ones(3, dtype), nnz_test=3, K=2, p=np.full(M, 7.0, dtype), ndcg=np.full(M, 7.0, dtype))
    kw.update(change)
    lib = hip.load()
    fn = getattr(lib, "rm_calc_metrics_candidates_%s%s" % ("dev_" if dev else "", "f32" if dtype == np.float32 else "f64"))
    outs = [_p(kw["p"])] + [None] * 4 + [_p(kw["ndcg"])] + [None] * 4
    rc = fn(_p(kw["A"]), kw["lda"], _p(kw["B"]), kw["ldb"], kw["m"], kw["n"], kw["k"], _p(kw["cp"]), _p(kw["ci"]), *((C.c_int64(kw["nnz"]),) if dev else ()),
            _p(kw["tp"]), _p(kw["ti"]), _p(kw["tv"]), *((C.c_int64(kw["nnz_test"]),) if dev else ()), kw["K"], 0, *outs, 2, 1, None if dev else 1)
    return rc, (lib.rm_last_error() or b"").decode(), all((kw[name] == 7.0).all() for name in ("p", "ndcg"))


CASES = {"null A": dict(A=None), "null B": dict(B=None), "null Xcand_csr_p": dict(cp=None), "null Xtest_csr_p": dict(tp=None), "null Xtest_csr_i": dict(ti=None),
         "NDCG without test values": dict(tv=None), "n <= 0": dict(n=0), "k <= 0": dict(k=0), "m < 0": dict(m=-1), "k_metrics < 1": dict(K=0),
         "lda < k": dict(lda=KF - 1)}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_what_the_host_decides(hip, dtype, dev):
    descending = dict(cp=np.array([0, 4, 2, 6], np.int32))
    for what, change in dict(CASES, **({"nnz_cand < 0": dict(nnz=-1), "nnz_test < 0": dict(nnz_test=-1)} if dev else {"descending index pointers": descending})).items():
        rc, msg, untouched = _call(hip, dtype, dev, **change)
        assert rc == RM_ERR_INVALID and msg and untouched, what
    assert "row 1" in _call(hip, dtype, False, **descending)[1]
    rc, msg, untouched = _call(hip, dtype, dev, K=1025)
    assert rc == RM_ERR_UNSUPPORTED and "1024" in msg and untouched
    long_row = dict(cp=np.array([0, 2, 2051, 2053], np.int32), ci=np.zeros(2053, np.int32), nnz=2053)      # (host entry: decided from the index pointers)
    rc, msg, untouched = _call(hip, dtype, False, **long_row)
    assert rc == RM_ERR_UNSUPPORTED and "candidate row 1 has more than 2048 entries" in msg and "sweep" in msg and untouched
    assert _call(hip, dtype, dev, m=0)[::2] == (RM_OK, True)
    if hip.device_count() == 0:                                       # without a device the call raises rather than computing on the CPU
        rc, msg, untouched = _call(hip, dtype, dev)
        assert rc not in (RM_OK, RM_ERR_INVALID, RM_ERR_UNSUPPORTED) and msg and untouched


def test_the_public_function_before_it_reaches_the_library(monkeypatch):
    import torch
    from scipy.sparse import csr_array
    from recometrics_amd import _binding, calc_reco_metrics_from_candidates as calc
    A, B = np.ones((M, KF), np.float32), np.ones((N, KF), np.float32)
    X = csr_array((np.ones(3, np.float32), np.array([0, 1, 5], np.int32), np.array([0, 1, 2, 3], np.int32)), shape=(M, N))
    pair = (np.array([0, 2, 4, 5], np.int32), np.array([0, 3, 1, 3, 4], np.int32))      # user 2's test item 5 is not among its candidates
    for bad, message in ((dict(A=A[:2]), "users in 'A' and 'X_test'"), (dict(B=B[:5]), "items in 'B' and 'X_test'"),
                         (dict(candidates=(pair[0][:3], pair[1])), "users in 'A' and 'candidates'"),
                         (dict(candidates=csr_array((M, N + 1))), "items in 'B' and 'candidates'"), (dict(k=0), "'k' must be positive"),
                         (dict(A=torch.ones((M, KF), dtype=torch.float16), B=torch.ones((N, KF), dtype=torch.float16)), "16-bit factors are not supported"),
                         (dict(A=torch.ones((M, KF), dtype=torch.bfloat16), B=torch.ones((N, KF), dtype=torch.bfloat16)), "16-bit factors are not supported"),
                         ({}, "user 2 has a test item that is not among its candidates")):
        with pytest.raises(ValueError, match=message):
            calc(**dict(dict(X_test=X, A=A, B=B, candidates=pair), **bad))
    class Reached(Exception):
        pass

    def binding(A, lda, B, ldb, cand_p, cand_i, *rest, **kw):
        raise Reached(cand_p.tolist(), cand_i.tolist())
    monkeypatch.setattr(_binding, "calc_metrics_candidates", binding)
    with pytest.raises(Reached) as reached:
        calc(X, A, B, pair, add_test_items=True)
    assert reached.value.args == ([0, 2, 4, 6], [0, 3, 1, 3, 4, 5])   # the union, row by row
