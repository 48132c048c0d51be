"""CPU-only: the C-ABI library is built, loads, and exports every symbol include/recometrics_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "recometrics_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rm_[a-z0-9_]+)\s*\(", text)))


def _declarations():
    """symbol -> (return type, [(parameter type, parameter name)]) of every rm_* declaration of the header"""
    text = open(os.path.join(ROOT, "include", "recometrics_hip.h")).read()
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    found = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [] if params.strip() == "void" else [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        found[name] = (" ".join(ret.split()), [(" ".join(t.split()), n) for t, n in params])
    return found


def _c_kind(ctype):
    """a C type of the header by kind and width"""
    if "*" in ctype:
        return "char *" if ctype == "const char *" else "pointer"
    return {"void": "void", "double": "double", "int": ("signed", 4), "int32_t": ("signed", 4), "int64_t": ("signed", 8),
            "uint64_t": ("unsigned", 8), "size_t": ("unsigned", 8)}[ctype.replace("const ", "")]


def _ctypes_kind(t):
    """a ctypes type by kind and width, not by class: c_int32 is c_int and c_uint64 is c_size_t here"""
    if t is None:
        return "void"
    if t is ctypes.c_char_p:
        return "char *"
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "pointer"
    if t is ctypes.c_double:
        return "double"
    assert issubclass(t, ctypes._SimpleCData) and t._type_ in "iIlLqQ", t
    return ("unsigned" if t(-1).value > 0 else "signed", ctypes.sizeof(t))


def test_the_binding_states_every_declaration_of_the_header():
    """_binding.SIGNATURES against include/recometrics_hip.h: the same symbols, and per symbol the same parameter names in the same
    order, every type of the same kind and width (an int32 where the header says int64_t, or two neighbours swapped, fails here)"""
    from recometrics_amd import _binding
    declared = _declarations()
    assert len(declared) == 45 and {"rm_debug_ws_check", "rm_debug_ws_poke"} <= set(declared) and sorted(declared) == _declared_symbols()
    assert set(_binding.SIGNATURES) == set(declared) and _binding.EXPORTS == tuple(_binding.SIGNATURES)
    for name, (ret, params) in declared.items():
        mine, restype = _binding.SIGNATURES[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(t) for t, _ in params], name
        assert _ctypes_kind(restype) == _c_kind(ret), name


def test_the_invoker_refuses_a_missing_or_unknown_name_before_the_call(monkeypatch):
    import numpy as np
    from recometrics_amd import _binding
    monkeypatch.setattr(_binding, "load", lambda: pytest.fail("the library was reached"))
    values = dict(A=None, lda=4, B=None, ldb=4, m=2, n=8, k=4, out=None)
    with pytest.raises(KeyError, match="ldb"):
        _binding._invoke("rm_debug_scores", np.float32, **{name: v for name, v in values.items() if name != "ldb"})
    with pytest.raises(TypeError, match="rm_debug_scores_f64 has no parameter lds, seed"):
        _binding._invoke("rm_debug_scores", np.float64, seed=1, lds=8, **values)


def test_header_declares_the_reference_boundary():
    syms = _declared_symbols()
    for must in ("rm_calc_metrics_f32", "rm_calc_metrics_f64", "rm_has_openmp", "rm_last_error"):
        assert must in syms


def test_library_builds_and_exports_every_declared_symbol():
    from recometrics_amd import build as rb
    path = rb.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    for sym in _declared_symbols():
        assert hasattr(lib, sym), "missing export: " + sym
    # host-only calls that need no GPU
    lib.rm_last_error.restype = ctypes.c_char_p
    assert lib.rm_has_openmp() == 1
    assert lib.rm_device_count() >= 0
    assert lib.rm_last_error() is not None


def test_the_library_is_built_from_the_sources_as_they_are():
    """build() decides on content, and records what it compiled: the digest in csrc/build_stamp.json must be the digest of the
    sources in the tree (a stale .so next to newer sources -- or next to a reverted file with an old mtime -- is rebuilt)"""
    from recometrics_amd import build as rb
    rb.build()
    st = rb.read_stamp()
    assert st is not None and st["sources_sha256"] == rb.sources_digest()
    assert st["library_bytes"] == os.path.getsize(rb.LIB) and not rb.needs_build()
    assert set(st["translation_units"]) == set(rb.SOURCES)


def test_no_device_is_a_loud_error_not_a_fallback():
    """Without a GPU the product path must raise (status != 0, message set), never compute on the CPU."""
    import numpy as np
    from recometrics_amd import _binding
    if _binding.device_count() > 0:
        pytest.skip("a GPU is present")
    A = np.ones((2, 4), np.float32)
    B = np.ones((8, 4), np.float32)
    p = np.array([0, 1, 2], np.int32)
    i = np.array([1, 2], np.int32)
    with pytest.raises((RuntimeError, MemoryError)):
        _binding.rank(A, B, np.zeros(3, np.int32), np.zeros(0, np.int32), p, i, 2)


def test_product_never_imports_the_oracle():
    """recometrics_amd/ must not import, include, link or dlopen anything under oracle/."""
    pkg = os.path.join(ROOT, "recometrics_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith((".py", ".hip", ".hpp", ".h")):
                continue
            for line in open(os.path.join(dirpath, f), errors="replace"):
                low = line.lower()
                if "oracle" in low and ("import" in low or "#include" in low or "cdll" in low or "dlopen" in low):
                    raise AssertionError("%s references the oracle: %s" % (f, line.strip()))


def test_cython_binding_builds_and_imports():
    """recometrics_amd/_cy.pyx compiles against include/recometrics_hip.h and links to the library (no GPU needed)"""
    from recometrics_amd import build as rb
    path = rb.build_cython()
    assert os.path.exists(path)
    from recometrics_amd import _cy
    assert _cy.has_openmp() is True
    assert _cy.device_count() >= 0
    assert _cy.METRIC_ORDER == ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr")
