"""CPU-only: the test hooks the library exports beside the header's API (_binding.TEST_HOOKS) against their C definitions.

include/recometrics_hip.h declares the API and tests/test_cabi_exports.py holds _binding.SIGNATURES to it; a hook that is not part of
the API is defined in csrc/rm_lib.hip alone, so its statement in Python is held to that definition here: the same parameter names
in the same order, every type of the same kind and width, the same return type -- and the built library exports the symbol."""
import ctypes
import os
import re

from test_cabi_exports import _c_kind, _ctypes_kind, _declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _definitions():
    """symbol -> (return type, [(parameter type, parameter name)]) of every extern "C" rm_* definition of csrc/rm_lib.hip"""
    text = open(os.path.join(ROOT, "recometrics_amd", "csrc", "rm_lib.hip")).read()
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for ret, name, params in re.findall(r'extern "C"\s+([\w\s\*]+?)\b(rm_\w+)\s*\(([^)]*)\)\s*\{', text):
        params = [] if params.strip() == "void" else [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        found[name] = (" ".join(ret.split()), [(" ".join(t.split()), n) for t, n in params])
    return found


def test_every_hook_is_stated_as_it_is_defined():
    from recometrics_amd import _binding
    defined = _definitions()
    assert "rm_get_timings" in defined and "rm_debug_reload_switches" in defined, "the scan of rm_lib.hip is stale"
    assert _binding.TEST_HOOKS, "no hook is stated"
    for name, (mine, restype) in _binding.TEST_HOOKS.items():
        assert name not in _binding.SIGNATURES and name not in _declared_symbols(), "%s is part of the header's API: state it there" % name
        assert name in defined, "%s is not defined in csrc/rm_lib.hip" % name
        ret, params = defined[name]
        assert [n for n, _ in mine] == [n for _, n in params], name
        assert [_ctypes_kind(t) for _, t in mine] == [_c_kind(t) for t, _ in params], name
        assert _ctypes_kind(restype) == _c_kind(ret), name


def test_the_library_exports_every_hook():
    from recometrics_amd import _binding, build as rb
    lib = ctypes.CDLL(rb.build())
    for name in _binding.TEST_HOOKS:
        assert hasattr(lib, name), "missing export: " + name
