"""CPU-only: the factor entries for 16-bit factor matrices (include/recometrics_hip_half_factors.h: rm_calc_metrics_{f16,bf16},
rm_recommend_{f16,bf16} and their _dev forms) and `A` / `B` as torch.Tensors -- what is decided without a device: the header against
_binding.HALF_FACTOR_SIGNATURES, the exports, m == 0, every RM_ERR_INVALID case with the _f32 entry's message, "no device is an error,
not a fallback", and what reaches the binding for CPU tensors.  (What the entries compute is tests/test_hip_factors_half.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_scores_half_cpu import _c_kind, _ctypes_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_OK, RM_ERR_INVALID, RM_ERR_HIP = 0, 1, 2
KINDS = ("f16", "bf16")
SYMBOLS = tuple("rm_%s%s_%s" % (request, form, kind) for request in ("calc_metrics", "recommend") for form in ("", "_dev") for kind in KINDS)
M, N, KF = 3, 8, 4


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import build as rb
    rb.build()
    from recometrics_amd import _binding
    _binding.load()
    return _binding


# ---- the header against the binding's table ------------------------------------------------------------------------------------------
def _declarations():
    """symbol -> (return type, [(parameter type, parameter name)]) of every rm_* declaration of the header, in its order"""
    text = open(os.path.join(ROOT, "include", "recometrics_hip_half_factors.h")).read()
    assert "double" not in text
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    found = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        found[name] = (" ".join(ret.split()), [(" ".join(t.split()), n) for t, n in params])
    return found


def test_the_binding_states_every_declaration_of_the_half_factor_header():
    from recometrics_amd import _binding
    declared = _declarations()
    table = _binding.HALF_FACTOR_SIGNATURES
    assert len(declared) == 8 and sorted(declared) == sorted(SYMBOLS) and set(table) == set(declared)
    assert not set(table) & set(_binding.SIGNATURES) and not set(table) & set(_binding.HALF_SIGNATURES)
    assert _binding.EXPORTS == tuple(_binding.SIGNATURES)
    for name, (ret, params) in declared.items():
        mine, restype = table[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(t.replace("uint64_t", "size_t")) for t, _ in params], name
        assert ret == "int" and _ctypes_kind(restype) == ("signed", 4), name
        assert params[0] == ("const uint16_t *", "A") and params[1] == ("size_t", "lda"), name
        assert params[2] == ("const uint16_t *", "B") and params[3] == ("size_t", "ldb"), name
        twin, _ = _binding.SIGNATURES[name.rsplit("_", 1)[0] + "_f32"]
        assert [n for n, _ in mine] == [n for n, _ in twin], name             # the parameter list of the _f32 entry, name for name
        assert [_ctypes_kind(t) for _, t in mine] == [_ctypes_kind(t) for _, t in twin], name
        for ctype, pname in params[4:]:
            assert "double" not in ctype and "uint16_t" not in ctype, (name, pname)
            if pname in _binding.OUTPUTS or pname in ("score", "Xtest_csr"):
                assert ctype.replace("const ", "") == "float *", (name, pname)
    half = open(os.path.join(ROOT, "include", "recometrics_hip_half.h")).read()
    assert "recometrics_hip_half_factors.h" in half and "There is no 16-bit form of the factor entries" not in half


def test_the_library_exports_all_eight(hip):
    lib = hip.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), "missing export: " + sym
        assert getattr(lib, sym).argtypes == [t for _, t in hip.HALF_FACTOR_SIGNATURES[sym][0]]
    for name in ("calc_metrics_half", "calc_metrics_half_device", "recommend_half", "recommend_half_device"):
        assert callable(getattr(hip, name))


# ---- the raw entries, each next to its _f32 twin -------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _inputs():
    A = np.arange(M * KF, dtype=np.float32).reshape(M, KF).astype(np.float16).view(np.uint16)     # (finite patterns in either format)
    B = np.arange(N * KF, dtype=np.float32).reshape(N, KF).astype(np.float16).view(np.uint16)
    trp, tri = np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)
    tep, tei, tev = np.array([0, 1, 2, 3], np.int32), np.array([4, 5, 6], np.int32), np.ones(3, np.float32)
    return dict(A=A, B=B, lda=KF, ldb=KF, m=M, n=N, k=KF, K=2, trp=trp, tri=tri, tep=tep, tei=tei, tev=tev, nnz=(3, 3), xp=None, xi=None, xnnz=0)


def _wide(x):
    return None if x is None else np.zeros(x.shape, np.float32)


def _lists(hip, suffix, dev, kw, idx, sc, st):
    lib = hip.load()
    fn = getattr(lib, "rm_recommend_%s%s" % ("dev_" if dev else "", suffix))
    A, B = (kw["A"], kw["B"]) if suffix != "f32" else (_wide(kw["A"]), _wide(kw["B"]))
    mid = (C.c_int64(kw["xnnz"]),) if dev else ()
    rc = fn(_p(A), kw["lda"], _p(B), kw["ldb"], kw["m"], kw["n"], kw["k"], _p(kw["xp"]), _p(kw["xi"]), *mid, kw["K"], _p(idx), _p(sc), _p(st),
            None if dev else 1)
    return rc, (lib.rm_last_error() or b"").decode()


def _metrics(hip, suffix, dev, kw, outs):
    lib = hip.load()
    fn = getattr(lib, "rm_calc_metrics_%s%s" % ("dev_" if dev else "", suffix))
    A, B = (kw["A"], kw["B"]) if suffix != "f32" else (_wide(kw["A"]), _wide(kw["B"]))
    train = (_p(kw["trp"]), _p(kw["tri"])) + ((C.c_int64(kw["nnz"][0]),) if dev else ())
    test = (_p(kw["tep"]), _p(kw["tei"]), _p(kw["tev"])) + ((C.c_int64(kw["nnz"][1]),) if dev else ())
    tail = (C.c_uint64(1), None) if dev else (1, C.c_uint64(1))
    rc = fn(_p(A), kw["lda"], _p(B), kw["ldb"], kw["m"], kw["n"], kw["k"], *train, *test, kw["K"], 0, 0, *[_p(o) for o in outs], 1, 2, 1, *tail)
    return rc, (lib.rm_last_error() or b"").decode()


def _list_outputs(K=2):
    return np.full((M, K), 77, np.int32), np.full((M, K), 7.0, np.float32), np.full(M, 77, np.int32)


def _metric_outputs():
    return [np.full(M, 7.0, np.float32) for _ in range(10)]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_no_user_is_ok_and_writes_nothing(hip, kind, dev):
    kw = dict(_inputs(), m=0)
    idx, sc, st = _list_outputs()
    rc, _ = _lists(hip, kind, dev, kw, idx, sc, st)
    assert rc == RM_OK and (idx == 77).all() and (sc == 7.0).all() and (st == 77).all()
    outs = _metric_outputs()
    rc, _ = _metrics(hip, kind, dev, kw, outs)
    assert rc == RM_OK and all((o == 7.0).all() for o in outs)


LIST_CASES = {"null A": dict(A=None), "null B": dict(B=None), "lda < k": dict(lda=KF - 1), "ldb < k": dict(ldb=KF - 1), "n <= 0": dict(n=0),
              "n < 0": dict(n=-3), "m < 0": dict(m=-1), "k <= 0": dict(k=0), "k_top = 0": dict(K=0), "k_top = n + 1": dict(K=N + 1),
              "null idx": "idx", "null status": "st"}


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_invalid_list_requests_are_decided_without_a_device(hip, kind, dev):
    """every host-decided case of the _f32 entry: the same status, the same message, nothing written"""
    cases = dict(LIST_CASES)
    if dev:
        cases.update({"negative nnz_excl": dict(xp=np.array([0, 1, 2, 3], np.int32), xi=np.array([0, 1, 2], np.int32), xnnz=-1),
                      "null excl indices": dict(xp=np.array([0, 1, 2, 3], np.int32), xi=None, xnnz=3)})
    else:
        cases.update({"decreasing pointers": dict(xp=np.array([0, 2, 1, 3], np.int32), xi=np.array([0, 1, 2], np.int32)),
                      "null excl indices": dict(xp=np.array([0, 1, 2, 3], np.int32), xi=None)})
    for what, change in cases.items():
        idx, sc, st = _list_outputs()
        kw = dict(_inputs(), **(change if isinstance(change, dict) else {}))
        outs = [None if change == "idx" else idx, sc, None if change == "st" else st]
        rc, msg = _lists(hip, kind, dev, kw, *outs)
        want_rc, want_msg = _lists(hip, "f32", dev, kw, *outs)
        assert rc == RM_ERR_INVALID == want_rc and msg and msg == want_msg, (what, rc, msg, want_rc, want_msg)
        assert (idx == 77).all() and (sc == 7.0).all() and (st == 77).all(), what


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_invalid_metric_requests_are_decided_without_a_device(hip, kind, dev):
    cases = {"null A": dict(A=None), "null B": dict(B=None), "lda < k": dict(lda=KF - 1), "ldb < k": dict(ldb=KF - 1), "n <= 0": dict(n=0),
             "k <= 0": dict(k=0), "k_metrics = 0": dict(K=0), "null train pointers": dict(trp=None),
             "null test pointers": dict(tep=None), "null test indices": dict(tei=None), "NDCG without values": dict(tev=None)}
    if dev:
        cases["m < 0"] = dict(m=-1)
    else:
        cases.update({"m < 0": dict(m=-1), "decreasing pointers": dict(trp=np.array([0, 2, 1, 3], np.int32)),
                      "null train indices": dict(tri=None)})
    for what, change in cases.items():
        outs = _metric_outputs()
        kw = dict(_inputs(), **change)
        rc, msg = _metrics(hip, kind, dev, kw, outs)
        want_rc, want_msg = _metrics(hip, "f32", dev, kw, outs)
        assert rc == RM_ERR_INVALID == want_rc and msg and msg == want_msg, (what, rc, msg, want_rc, want_msg)
        assert all((o == 7.0).all() for o in outs), what


@pytest.mark.parametrize("kind", KINDS)
def test_no_device_is_an_error_not_a_fallback(hip, kind):
    if hip.device_count() > 0:
        pytest.skip("a GPU is present")
    kw = _inputs()
    for dev in (False, True):
        idx, sc, st = _list_outputs()
        outs = _metric_outputs()
        rc, msg = _lists(hip, kind, dev, kw, idx, sc, st)
        assert rc == RM_ERR_HIP and msg and (idx == 77).all() and (sc == 7.0).all() and (st == 77).all()
        rc, msg = _metrics(hip, kind, dev, kw, outs)
        assert rc == RM_ERR_HIP and msg and all((o == 7.0).all() for o in outs)
    as_arg = (lambda x: x.view(np.float16)) if kind == "f16" else (lambda x: x)
    with pytest.raises(RuntimeError):
        hip.recommend_half(as_arg(kw["A"]), KF, as_arg(kw["B"]), KF, None, None, 2)
    import torch
    from recometrics_amd import recommend_topk
    tdtype = torch.float16 if kind == "f16" else torch.bfloat16
    with pytest.raises(RuntimeError):
        recommend_topk(torch.ones(M, KF, dtype=tdtype), torch.ones(N, KF, dtype=tdtype), k=2)


# ---- `A`, `B` as CPU tensors: what reaches the binding -------------------------------------------------------------------------------
@pytest.fixture()
def seen(monkeypatch):
    """the four host wrappers of the binding record their arguments instead of calling the library"""
    from recometrics_amd import _binding
    calls = []

    def recorder(name):
        def fake(A, lda, B, ldb, *args, **kwargs):
            calls.append(dict(entry=name, A=A, lda=lda, B=B, ldb=ldb, args=args))
            return ("ids", "scores", "status") if name.startswith("recommend") else tuple(np.zeros(A.shape[0], np.float32) for _ in range(10))
        return fake
    for name in ("recommend", "recommend_half", "calc_metrics", "calc_metrics_half"):
        monkeypatch.setattr(_binding, name, recorder(name))
    monkeypatch.setattr(_binding, "load", lambda: pytest.fail("the library was reached"))
    monkeypatch.setattr(_binding, "has_openmp", lambda: True)
    return calls


def _test_matrix(m, n):
    from scipy.sparse import csr_array
    return csr_array((np.ones(m, np.float32), (np.arange(m), np.arange(m) % n)), shape=(m, n))


@pytest.mark.parametrize("which", ["lists", "metrics"])
@pytest.mark.parametrize("kind", KINDS)
def test_half_cpu_tensors_reach_the_binding_as_views(seen, kind, which):
    import torch
    from recometrics_amd import calc_reco_metrics, recommend_topk
    m, n, k = 4, 9, 6
    tdtype, ndtype = (torch.float16, np.float16) if kind == "f16" else (torch.bfloat16, np.uint16)
    entry = "recommend_half" if which == "lists" else "calc_metrics_half"

    def call(a, b, **kw):
        del seen[:]
        if which == "lists":
            assert recommend_topk(a, b, k=3, **kw) == ("ids", "scores", "status")
        else:
            calc_reco_metrics(None, _test_matrix(a.shape[0], b.shape[0]), a, b, k=3)
        assert len(seen) == 1 and seen[0]["entry"] == entry and seen[0]["A"].dtype == ndtype and seen[0]["B"].dtype == ndtype, seen
        return seen[0]

    wa, wb = torch.randn(m, k + 5).to(tdtype), torch.randn(n, k + 3).to(tdtype)
    va, vb = wa[:, 2:2 + k], wb[:, 1:1 + k]                                            # row strides: passed as they are
    got = call(va, vb)
    assert (got["lda"], got["ldb"]) == (k + 5, k + 3) and got["A"].shape == (m, k) and got["B"].shape == (n, k)
    assert got["A"].ctypes.data == va.data_ptr() == wa.data_ptr() + 4 and got["B"].ctypes.data == vb.data_ptr() == wb.data_ptr() + 2
    before = got["A"].copy()
    wa[1, 3] = 100.0                                                                    # shared memory: the view sees the write
    assert (got["A"] != before).sum() == 1 and (got["A"] != before)[1, 1]
    assert (got["A"].view(np.uint16) == va.contiguous().view(torch.int16).numpy().view(np.uint16)).all()
    assert (got["B"].view(np.uint16) == vb.contiguous().view(torch.int16).numpy().view(np.uint16)).all()
    da, db = torch.randn(m, k).to(tdtype), torch.randn(n, k).to(tdtype)                 # dense rows
    dense = call(da, db)
    assert (dense["lda"], dense["ldb"]) == (k, k) and dense["A"].ctypes.data == da.data_ptr() and dense["B"].ctypes.data == db.data_ptr()
    if which == "lists":
        got = call(va, vb, users=np.array([3, 0]))                                      # users=: one gather of rows of A
        assert got["lda"] == k and (got["A"].view(np.uint16) == va.contiguous().view(torch.int16).numpy().view(np.uint16)[[3, 0]]).all()
        assert got["B"].ctypes.data == vb.data_ptr()


@pytest.mark.parametrize("tname", ["float32", "float64"])
def test_float_cpu_tensors_take_the_numpy_entries(seen, tname):
    import torch
    from recometrics_amd import calc_reco_metrics, recommend_topk
    m, n, k = 4, 9, 6
    a, b = torch.randn(m, k + 2, dtype=getattr(torch, tname))[:, :k], torch.randn(n, k, dtype=getattr(torch, tname))
    recommend_topk(a, b, k=3)
    calc_reco_metrics(None, _test_matrix(m, n), a, b, k=3)
    assert [c["entry"] for c in seen] == ["recommend", "calc_metrics"]
    for c in seen:
        assert c["A"].dtype == np.dtype(tname) and c["lda"] == k + 2 and c["A"].ctypes.data == a.data_ptr() and c["B"].ctypes.data == b.data_ptr()
    del seen[:]
    bias = np.arange(n, dtype=np.float64)                                               # item_biases: one more column, by torch.cat
    recommend_topk(a, b, k=3, item_biases=bias)
    assert seen[0]["A"].shape == (m, k + 1) and (seen[0]["A"][:, k] == 1).all() and (seen[0]["B"][:, k] == bias).all()
    assert (seen[0]["A"][:, :k] == a.numpy()).all() and seen[0]["A"].dtype == np.dtype(tname)


def test_what_is_refused_and_what_stays_as_it_was(seen):
    import torch
    from recometrics_amd import calc_reco_metrics, recommend_topk
    m, n, k = 4, 9, 6
    X = _test_matrix(m, n)
    h, b16 = torch.ones(m, k, dtype=torch.float16), torch.ones(n, k, dtype=torch.bfloat16)
    calls = lambda A, B, **kw: (lambda: recommend_topk(A, B, k=3, **kw), lambda: calc_reco_metrics(None, X, A, B, k=3, **kw))
    for A, B in ((h, b16), (h, torch.ones(n, k)), (torch.ones(m, k, dtype=torch.float64), torch.ones(n, k))):       # mixed dtypes
        for call in calls(A, B):
            with pytest.raises(ValueError, match="same dtype"):
                call()
    for A, B in ((h, np.ones((n, k), np.float16)), (np.ones((m, k), np.float32), torch.ones(n, k))):                # a tensor next to an array
        for call in calls(A, B):
            with pytest.raises(ValueError, match="both be torch tensors"):
                call()
    for call in calls(h, torch.ones(n, k, dtype=torch.float16, device="meta")):                                    # mixed devices
        with pytest.raises(ValueError, match="same device"):
            call()
    for call in calls(torch.ones(m, k, dtype=torch.int32), torch.ones(n, k, dtype=torch.int32)):
        with pytest.raises(ValueError, match="float16, bfloat16, float32 or float64"):
            call()
    for tdtype in (torch.float16, torch.bfloat16):                                                                  # 16-bit factors with item_biases
        for call in calls(torch.ones(m, k, dtype=tdtype), torch.ones(n, k, dtype=tdtype), item_biases=np.ones(n)):
            with pytest.raises(ValueError, match="item_biases"):
                call()
    assert not seen
    # NumPy float16 arrays take today's path: through float64
    recommend_topk(np.ones((m, k), np.float16), np.ones((n, k), np.float16), k=3)
    calc_reco_metrics(None, X, np.ones((m, k), np.float16), np.ones((n, k), np.float16), k=3)
    assert [(c["entry"], c["A"].dtype, c["B"].dtype) for c in seen] == [("recommend", np.float64, np.float64), ("calc_metrics", np.float64, np.float64)]
    # a non-array still trips the assertion
    with pytest.raises(AssertionError):
        recommend_topk(np.ones((m, k)).tolist(), np.ones((n, k)).tolist(), k=3)
    with pytest.raises(AssertionError):
        calc_reco_metrics(None, X, np.ones((m, k)).tolist(), np.ones((n, k)).tolist(), k=3)
