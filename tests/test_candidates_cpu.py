"""CPU-only: lists from candidate sets (include/recometrics_hip_candidates.h, recommend_topk_from_candidates) -- what is decided without
a device: the header against _binding.CAND_SIGNATURES, the exports, m == 0, every host-decided RM_ERR_INVALID / RM_ERR_UNSUPPORTED with
the outputs untouched, and the public function's ValueErrors.  (What the entries compute is tests/test_hip_candidates.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_factors_half_cpu import _p, hip  # noqa: F401 (hip: a fixture -- the library, built)
from test_scores_half_cpu import _c_kind, _ctypes_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_OK, RM_ERR_INVALID, RM_ERR_UNSUPPORTED = 0, 1, 4
SYMBOLS = tuple("rm_recommend_candidates%s_%s" % (form, suffix) for form in ("", "_dev") for suffix in ("f32", "f64"))
M, N, KF = 3, 8, 4


def test_the_binding_states_every_declaration_of_the_header():
    from recometrics_amd import _binding
    text = open(os.path.join(ROOT, "include", "recometrics_hip_candidates.h")).read()
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    declared = re.findall(r"([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*;", text)
    table = _binding.CAND_SIGNATURES
    assert [name for _, name, _ in declared] == list(SYMBOLS) and set(table) == set(SYMBOLS) and not set(table) & set(_binding.SIGNATURES)
    for ret, name, params in declared:
        params = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        mine, restype = table[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(" ".join(t.split())) for t, _ in params], name
        assert ret.strip() == "int" and _ctypes_kind(restype) == ("signed", 4), name
        real = "double" if name.endswith("f64") else "float"
        assert [" ".join(t.split()) for t, n in params if n in ("A", "B", "score")] == ["const %s *" % real] * 2 + [real + " *"], name


def test_the_library_exports_all_four(hip):
    import recometrics_amd
    lib = hip.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), "missing export: " + sym
        assert getattr(lib, sym).argtypes == [t for _, t in hip.CAND_SIGNATURES[sym][0]]
    assert callable(hip.recommend_candidates) and callable(hip.recommend_candidates_device)
    assert "recommend_topk_from_candidates" in recometrics_amd.__all__


def _call(hip, dtype, dev, **change):
    """(status, message, outputs) of an entry on a small valid request with `change` applied; the outputs start as 77 / 7.0"""
    kw = dict(A=np.ones((M, KF), dtype), B=np.ones((N, KF), dtype), lda=KF, ldb=KF, m=M, n=N, k=KF, cp=np.array([0, 1, 2, 3], np.int32),
              ci=np.array([0, 1, 2], np.int32), nnz=3, K=2, idx=np.full((M, 2), 77, np.int32), sc=np.full((M, 2), 7.0, dtype), st=np.full(M, 77, np.int32))
    kw.update(change)
    lib = hip.load()
    fn = getattr(lib, "rm_recommend_candidates_%s%s" % ("dev_" if dev else "", "f32" if dtype == np.float32 else "f64"))
    rc = fn(_p(kw["A"]), kw["lda"], _p(kw["B"]), kw["ldb"], kw["m"], kw["n"], kw["k"], _p(kw["cp"]), _p(kw["ci"]), *((C.c_int64(kw["nnz"]),) if dev else ()),
            kw["K"], _p(kw["idx"]), _p(kw["sc"]), _p(kw["st"]), None if dev else 1)
    untouched = all((kw[name] == (77 if name != "sc" else 7.0)).all() for name in ("idx", "sc", "st") if kw[name] is not None)
    return rc, (lib.rm_last_error() or b"").decode(), untouched


CASES = {"null A": dict(A=None), "null B": dict(B=None), "null Xcand_csr_p": dict(cp=None), "null idx": dict(idx=None), "null status": dict(st=None),
         "n <= 0": dict(n=0), "k <= 0": dict(k=0), "m < 0": dict(m=-1), "k_top < 1": dict(K=0), "lda < k": dict(lda=KF - 1)}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_what_the_host_decides(hip, dtype, dev):
    descending = dict(cp=np.array([0, 2, 1, 3], np.int32))
    for what, change in dict(CASES, **({"nnz_cand < 0": dict(nnz=-1)} if dev else {"descending index pointers": descending})).items():
        rc, msg, untouched = _call(hip, dtype, dev, **change)
        assert rc == RM_ERR_INVALID and msg and untouched, what
    assert "row 1" in _call(hip, dtype, False, **descending)[1]
    rc, msg, untouched = _call(hip, dtype, dev, K=1025, idx=np.full((M, 1025), 77, np.int32), sc=None)
    assert rc == RM_ERR_UNSUPPORTED and "1024" in msg and untouched
    assert _call(hip, dtype, dev, m=0)[::2] == (RM_OK, True)


def test_value_errors_of_the_public_function():
    import torch
    from scipy.sparse import csr_array
    from recometrics_amd import recommend_topk_from_candidates as reco
    A, B = np.ones((M, KF), np.float32), np.ones((N, KF), np.float32)
    pair = (np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32))
    for bad, message in ((dict(A=A[:2]), "users in 'A' and 'candidates'"), (dict(A=A[:2], candidates=csr_array((M, N))), "users in 'A' and 'candidates'"),
                         (dict(candidates=csr_array((M, N + 1))), "items in 'B' and 'candidates'"), (dict(k=0), "'k' must be positive"),
                         (dict(A=torch.ones((M, KF), dtype=torch.float16), B=torch.ones((N, KF), dtype=torch.float16)), "16-bit factors are not supported"),
                         (dict(A=torch.ones((M, KF), dtype=torch.bfloat16), B=torch.ones((N, KF), dtype=torch.bfloat16)), "16-bit factors are not supported")):
        with pytest.raises(ValueError, match=message):
            reco(**dict(dict(A=A, B=B, candidates=pair), **bad))
