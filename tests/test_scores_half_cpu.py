"""CPU-only: the from-scores entries for 16-bit score matrices (include/recometrics_hip_half.h: rm_calc_metrics_scores_{f16,bf16},
rm_recommend_scores_{f16,bf16} and their _dev forms) and `scores` as a torch.Tensor -- what is decided without a device: the header
against _binding.HALF_SIGNATURES, the exports, m == 0, every RM_ERR_INVALID case, "no device is an error, not a fallback", and what
reaches the binding for a CPU tensor.  (What the entries compute is tests/test_hip_scores_half.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_OK, RM_ERR_INVALID, RM_ERR_HIP = 0, 1, 2
KINDS = ("f16", "bf16")
SYMBOLS = tuple("rm_%s_scores%s_%s" % (request, form, kind) for request in ("calc_metrics", "recommend") for form in ("", "_dev") for kind in KINDS)


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
    text = open(os.path.join(ROOT, "include", "recometrics_hip_half.h")).read()
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    found = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        found[name] = (" ".join(ret.split()), [(" ".join(t.split()), n) for t, n in params])
    return found


def _c_kind(ctype):
    if "*" in ctype:
        return "pointer"
    return {"int": ("signed", 4), "int32_t": ("signed", 4), "int64_t": ("signed", 8), "size_t": ("unsigned", 8)}[ctype.replace("const ", "")]


def _ctypes_kind(t):
    if t is C.c_void_p or issubclass(t, C._Pointer):
        return "pointer"
    assert issubclass(t, C._SimpleCData) and t._type_ in "iIlLqQ", t
    return ("unsigned" if t(-1).value > 0 else "signed", C.sizeof(t))


def test_the_binding_states_every_declaration_of_the_half_header():
    """names, order, kinds and widths, as tests/test_cabi_exports.py holds _binding.SIGNATURES to the main header; and the element
    types the header promises: S in uint16_t, everything else the _f32 entry's"""
    from recometrics_amd import _binding
    declared = _declarations()
    assert sorted(declared) == sorted(SYMBOLS) and set(_binding.HALF_SIGNATURES) == set(declared)
    assert not set(_binding.HALF_SIGNATURES) & set(_binding.SIGNATURES) and _binding.EXPORTS == tuple(_binding.SIGNATURES)
    for name, (ret, params) in declared.items():
        mine, restype = _binding.HALF_SIGNATURES[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(t) for t, _ in params], name
        assert ret == "int" and _ctypes_kind(restype) == ("signed", 4), name
        assert params[0] == ("const uint16_t *", "S") and params[1] == ("size_t", "lds"), name
        twin, _ = _binding.SIGNATURES[name.rsplit("_", 1)[0] + "_f32"]
        assert [n for n, _ in mine] == [n for n, _ in twin], name             # the parameter list of the _f32 entry
        for ctype, pname in params[1:]:
            assert "double" not in ctype and "uint16_t" not in ctype, (name, pname)
            if pname in _binding.OUTPUTS or pname in ("score", "Xtest_csr"):
                assert ctype.replace("const ", "") == "float *", (name, pname)
    main = open(os.path.join(ROOT, "include", "recometrics_hip.h")).read()
    assert not re.search(r"rm_\w+_(b?f16)\b", main), "the 16-bit entries belong to recometrics_hip_half.h"


def test_the_library_exports_all_eight(hip):
    lib = hip.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), "missing export: " + sym
        assert getattr(lib, sym).argtypes == [t for _, t in hip.HALF_SIGNATURES[sym][0]]
    for name in ("calc_metrics_scores_half", "calc_metrics_scores_half_device", "recommend_scores_half", "recommend_scores_half_device"):
        assert callable(getattr(hip, name))


# ---- the raw entries -----------------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


M, N = 3, 8


def _inputs():
    S = np.arange(M * N, dtype=np.float32).reshape(M, N).astype(np.float16).view(np.uint16)      # (finite patterns in either format)
    trp, tri = np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)
    tep, tei, tev = np.array([0, 1, 2, 3], np.int32), np.array([4, 5, 6], np.int32), np.ones(3, np.float32)
    return S, trp, tri, tep, tei, tev


def _list_outputs(K=2):
    return np.full((M, K), 77, np.int32), np.full((M, K), 7.0, np.float32), np.full(M, 77, np.int32)


def _lists(hip, kind, dev, S, lds, m, n, K, idx, sc, st, xp=None, xi=None, nnz=0):
    lib = hip.load()
    fn = getattr(lib, "rm_recommend_scores_%s%s" % ("dev_" if dev else "", kind))
    tail = (None,) if dev else (1,)
    mid = (C.c_int64(nnz),) if dev else ()
    rc = fn(_p(S), lds, m, n, _p(xp), _p(xi), *mid, K, _p(idx), _p(sc), _p(st), *tail)
    return rc, (lib.rm_last_error() or b"").decode()


def _metrics(hip, kind, dev, S, lds, m, n, K, outs, trp, tri, tep, tei, tev, nnz=(3, 3)):
    lib = hip.load()
    fn = getattr(lib, "rm_calc_metrics_scores_%s%s" % ("dev_" if dev else "", kind))
    train = (_p(trp), _p(tri)) + ((C.c_int64(nnz[0]),) if dev else ())
    test = (_p(tep), _p(tei), _p(tev)) + ((C.c_int64(nnz[1]),) if dev else ())
    rc = fn(_p(S), lds, m, n, *train, *test, K, 0, *[_p(o) for o in outs], 1, 2, 1, None if dev else 1)
    return rc, (lib.rm_last_error() or b"").decode()


def _metric_outputs():
    return [np.full(M, 7.0, np.float32) for _ in range(10)]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_no_user_is_ok_and_writes_nothing(hip, kind, dev):
    S, trp, tri, tep, tei, tev = _inputs()
    idx, sc, st = _list_outputs()
    rc, _ = _lists(hip, kind, dev, S, N, 0, N, 2, idx, sc, st)
    assert rc == RM_OK and (idx == 77).all() and (sc == 7.0).all() and (st == 77).all()
    outs = _metric_outputs()
    rc, _ = _metrics(hip, kind, dev, S, N, 0, N, 2, outs, trp, tri, tep, tei, tev)
    assert rc == RM_OK and all((o == 7.0).all() for o in outs)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_invalid_list_requests_are_decided_without_a_device(hip, kind, dev):
    """the cases of the _f32 entry (tests/test_recommend_scores_cpu.py), with the _f32 entry's message"""
    S = _inputs()[0]
    W = np.zeros((M, N), np.float32)
    idx, sc, st = _list_outputs()
    cases = {"null S": dict(S=None), "lds < n": dict(lds=N - 1), "n <= 0": dict(n=0), "n < 0": dict(n=-3), "m < 0": dict(m=-1),
             "k_top = 0": dict(K=0), "k_top = n + 1": dict(K=N + 1), "null idx": dict(idx=None), "null status": dict(st=None)}
    f32 = getattr(hip.load(), "rm_recommend_scores_%sf32" % ("dev_" if dev else ""))
    for what, change in cases.items():
        kw = dict(S=S, lds=N, m=M, n=N, K=2, idx=idx, st=st)
        kw.update(change)
        rc, msg = _lists(hip, kind, dev, kw["S"], kw["lds"], kw["m"], kw["n"], kw["K"], kw["idx"], sc, kw["st"])
        assert rc == RM_ERR_INVALID and msg, (what, rc, msg)
        assert (idx == 77).all() and (sc == 7.0).all() and (st == 77).all(), what
        args = (_p(None if kw["S"] is None else W), kw["lds"], kw["m"], kw["n"], None, None) + ((C.c_int64(0),) if dev else ())
        assert f32(*args, kw["K"], _p(kw["idx"]), _p(sc), _p(kw["st"]), None if dev else 1) == RM_ERR_INVALID
        assert (hip.load().rm_last_error() or b"").decode() == msg, what
    if dev:
        xp, xi = np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)
        rc, msg = _lists(hip, kind, True, S, N, M, N, 2, idx, sc, st, xp=xp, xi=xi, nnz=-1)
        assert rc == RM_ERR_INVALID and msg and (idx == 77).all() and (st == 77).all()
    else:
        xp, xi = np.array([0, 2, 1, 3], np.int32), np.array([0, 1, 2], np.int32)
        rc, msg = _lists(hip, kind, False, S, N, M, N, 2, idx, sc, st, xp=xp, xi=xi)
        assert rc == RM_ERR_INVALID and "row 1" in msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_invalid_metric_requests_are_decided_without_a_device(hip, kind, dev):
    S, trp, tri, tep, tei, tev = _inputs()
    outs = _metric_outputs()
    base = dict(S=S, lds=N, m=M, n=N, K=2, trp=trp, tri=tri, tep=tep, tei=tei, tev=tev, nnz=(3, 3))
    cases = {"null S": dict(S=None), "lds < n": dict(lds=N - 1), "n <= 0": dict(n=0), "m < 0": dict(m=-1), "k_metrics = 0": dict(K=0),
             "k_metrics = n + 1": dict(K=N + 1), "null train pointers": dict(trp=None), "null test pointers": dict(tep=None),
             "null test indices": dict(tei=None), "NDCG without values": dict(tev=None)}
    if dev:
        cases.update({"negative nnz_train": dict(nnz=(-1, 3)), "negative nnz_test": dict(nnz=(3, -1))})
    else:
        cases.update({"decreasing pointers": dict(trp=np.array([0, 2, 1, 3], np.int32))})
    for what, change in cases.items():
        kw = dict(base)
        kw.update(change)
        rc, msg = _metrics(hip, kind, dev, kw["S"], kw["lds"], kw["m"], kw["n"], kw["K"], outs, kw["trp"], kw["tri"], kw["tep"], kw["tei"],
                           kw["tev"], kw["nnz"])
        assert rc == RM_ERR_INVALID and msg, (what, rc, msg)
        assert all((o == 7.0).all() for o in outs), what


@pytest.mark.parametrize("kind", KINDS)
def test_no_device_is_an_error_not_a_fallback(hip, kind):
    if hip.device_count() > 0:
        pytest.skip("a GPU is present")
    S, trp, tri, tep, tei, tev = _inputs()
    idx, sc, st = _list_outputs()
    outs = _metric_outputs()
    for dev in (False, True):
        rc, msg = _lists(hip, kind, dev, S, N, M, N, 2, idx, sc, st)
        assert rc == RM_ERR_HIP and msg and (idx == 77).all() and (sc == 7.0).all() and (st == 77).all()
        rc, msg = _metrics(hip, kind, dev, S, N, M, N, 2, outs, trp, tri, tep, tei, tev)
        assert rc == RM_ERR_HIP and msg and all((o == 7.0).all() for o in outs)
    half = S.view(np.float16) if kind == "f16" else S
    with pytest.raises(RuntimeError):
        hip.recommend_scores_half(half, N, None, None, 2)
    import torch
    from recometrics_amd import recommend_topk_from_scores
    with pytest.raises(RuntimeError):
        recommend_topk_from_scores(torch.from_numpy(S.view(np.float16)).view(torch.float16 if kind == "f16" else torch.bfloat16), k=2)


# ---- `scores` as a CPU tensor: what reaches the binding ------------------------------------------------------------------------------
@pytest.fixture()
def seen(monkeypatch):
    """the four host wrappers of the binding record their arguments instead of calling the library"""
    from recometrics_amd import _binding
    calls = []

    def recorder(name):
        def fake(S, lds, *args, **kwargs):
            calls.append(dict(entry=name, S=S, lds=lds, args=args))
            return ("ids", "scores", "status") if name.startswith("recommend") else tuple(np.zeros(S.shape[0], np.float32) for _ in range(10))
        return fake
    for name in ("recommend_scores", "recommend_scores_half", "calc_metrics_scores", "calc_metrics_scores_half"):
        monkeypatch.setattr(_binding, name, recorder(name))
    monkeypatch.setattr(_binding, "load", lambda: pytest.fail("the library was reached"))
    return calls


def _test_matrix(m, n):
    from scipy.sparse import csr_array
    return csr_array((np.ones(m, np.float32), (np.arange(m), np.arange(m) % n)), shape=(m, n))


@pytest.mark.parametrize("which", ["lists", "metrics"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_half_cpu_tensor_reaches_the_binding_as_a_view(seen, kind, which):
    import torch
    from recometrics_amd import calc_reco_metrics_from_scores, recommend_topk_from_scores
    m, n = 4, 9
    tdtype, ndtype = (torch.float16, np.float16) if kind == "f16" else (torch.bfloat16, np.uint16)
    entry = "recommend_scores_half" if which == "lists" else "calc_metrics_scores_half"

    def call(t, **kw):
        del seen[:]
        if which == "lists":
            assert recommend_topk_from_scores(t, k=3, **kw) == ("ids", "scores", "status")
        else:
            calc_reco_metrics_from_scores(None, _test_matrix(t.shape[0], t.shape[1]), t, k=3)
        assert len(seen) == 1 and seen[0]["entry"] == entry and seen[0]["S"].dtype == ndtype, seen
        return seen[0]

    wide = torch.randn(m, n + 5).to(tdtype)
    got = call(wide)                                                                   # dense rows
    assert got["lds"] == n + 5 and got["S"].shape == (m, n + 5) and got["S"].ctypes.data == wide.data_ptr()
    view = wide[:, 2:2 + n]                                                            # a row stride: passed as it is
    got = call(view)
    assert view.stride() == (n + 5, 1) and got["lds"] == view.stride(0) and got["S"].shape == (m, n)
    assert got["S"].ctypes.data == view.data_ptr() == wide.data_ptr() + 4
    before = got["S"].copy()
    wide[1, 3] = 100.0                                                                  # shared memory: the view sees the write
    assert (got["S"] != before).sum() == 1 and (got["S"] != before)[1, 1]
    bits = got["S"].view(np.uint16)
    want = view.contiguous().view(torch.int16).numpy().view(np.uint16)
    assert (bits == want).all()
    tr = wide[:, :m].t()                                                               # transposed: copied once, row-major
    assert tr.shape == (m, m) and tr.stride(1) != 1
    if which == "lists":
        got = call(tr)
        assert got["lds"] == m and got["S"].flags["C_CONTIGUOUS"] and got["S"].ctypes.data != tr.data_ptr()
        assert (got["S"].view(np.uint16) == tr.contiguous().view(torch.int16).numpy().view(np.uint16)).all()
        got = call(view, users=np.array([3, 0]))                                       # users=: one gather
        assert got["lds"] == n and (got["S"].view(np.uint16) == want[[3, 0]]).all()


@pytest.mark.parametrize("tname", ["float32", "float64"])
def test_a_float_cpu_tensor_takes_the_numpy_entries(seen, tname):
    import torch
    from recometrics_amd import calc_reco_metrics_from_scores, recommend_topk_from_scores
    m, n = 4, 9
    t = torch.randn(m, n + 2, dtype=getattr(torch, tname))[:, :n]
    recommend_topk_from_scores(t, k=3)
    calc_reco_metrics_from_scores(None, _test_matrix(m, n), t, k=3)
    assert [c["entry"] for c in seen] == ["recommend_scores", "calc_metrics_scores"]
    for c in seen:
        assert c["S"].dtype == np.dtype(tname) and c["lds"] == n + 2 and c["S"].ctypes.data == t.data_ptr()


def test_other_tensors_and_lists_raise_the_pinned_messages(seen):
    import torch
    from recometrics_amd import calc_reco_metrics_from_scores, recommend_topk_from_scores
    m, n = 4, 9
    X = _test_matrix(m, n)
    for bad in (torch.zeros(m, n, dtype=torch.complex64), torch.zeros(m, n, dtype=torch.int32), torch.zeros(m, n, dtype=torch.bool)):
        with pytest.raises(ValueError, match="^'scores' must be a numeric array.$"):
            recommend_topk_from_scores(bad, k=3)
        with pytest.raises(ValueError, match="^'scores' must be a numeric array.$"):
            calc_reco_metrics_from_scores(None, X, bad, k=3)
    with pytest.raises(ValueError, match="^'scores' must be a 2-dimensional array.$"):
        recommend_topk_from_scores(torch.zeros(n, dtype=torch.bfloat16), k=3)
    with pytest.raises(ValueError, match="^'scores' must be a NumPy array.$"):
        recommend_topk_from_scores(np.zeros((m, n)).tolist(), k=3)
    with pytest.raises(ValueError, match="^'scores' must be a NumPy array.$"):
        calc_reco_metrics_from_scores(None, X, np.zeros((m, n)).tolist(), k=3)
    assert not seen
    # a NumPy float16 array keeps going through float64
    recommend_topk_from_scores(np.ones((m, n), np.float16), k=3)
    calc_reco_metrics_from_scores(None, X, np.ones((m, n), np.float16), k=3)
    assert [(c["entry"], c["S"].dtype) for c in seen] == [("recommend_scores", np.float64), ("calc_metrics_scores", np.float64)]
