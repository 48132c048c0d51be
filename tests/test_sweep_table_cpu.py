"""CPU-only: the table of sweep-kernel instantiations (csrc/rm_sweep_units.hip) and the rule that picks a row for a request.

Which instantiation of k_sweep / k_sweep64 a call gets is a pure host function.  A wrong row does not show in the parity tests
where the variants agree bit for bit by design (the SPEC specialisations, the list schemes: only slower), and reads memory that
is not there where they do not (dense train rows under SPEC 1), so the selection is pinned here, against a restatement of the
rules written as data: nothing below is imported from the product but the three debug exports."""
import ctypes
import itertools

import pytest

LM_LDS, LM_HBM, LM_APPEND = 0, 1, 2
TO_64 = (2, 3, 4, 5, 6, 7, 8)                   # factor groups of 8
TO_128 = TO_64 + (10, 12, 13, 16)
ELEM = {"f32": 4, "f64": 8}


def _list_variants(ngs, spec, nsub=2, lmodes=(LM_LDS, LM_HBM, LM_APPEND)):
    return [(ng, auc, 0, lm, nsub, spec) for ng in ngs for auc in (0, 1) for lm in lmodes]


def _dumps(ngs):
    return [(ng, 0, 1, LM_HBM, 2, 0) for ng in ngs]


def expected_units():
    """the translation units and what each instantiates, keys = (ng, auc, dump, lmode, nsub, spec)"""
    f32, f64 = {}, {}
    for spec in (0, 1, 2):
        f32["n3_s%d" % spec] = _list_variants(TO_64, spec, nsub=3, lmodes=(LM_LDS,))
        f32["lds_s%d" % spec] = _list_variants(TO_128, spec, lmodes=(LM_LDS,))
        f32["hbm_s%d" % spec] = _list_variants(TO_128, spec, lmodes=(LM_HBM, LM_APPEND))
    f32["large"] = _list_variants((32, 64, 0), 0) + _dumps((32, 64, 0))
    f32["dump"] = _dumps(TO_128)
    for spec in (0, 1):
        f64["small_s%d" % spec] = _list_variants(TO_64, spec) + (_dumps(TO_64) if spec == 0 else [])
        f64["large_s%d" % spec] = _list_variants((16, 32, 64, 0), spec) + (_dumps((16, 32, 64, 0)) if spec == 0 else [])
    return {"f32": f32, "f64": f64}


def expected_key(prec, ng, ngt, auc, dump, lmode, nsub, spec):
    """the rules of the selection; None = unsupported"""
    if prec == "f32":
        if nsub == 3:
            if dump or lmode != LM_LDS or ng > 8 or ng not in TO_64:
                return None
            return (ng, auc, 0, LM_LDS, 3, spec)
        if ng > 16:
            if ng in (32, 64):
                tng = ng
            elif ng > 64 and ng % 16 == 0 and ng == ngt:
                tng = 0
            else:
                return None
            return (tng, 0, 1, LM_HBM, 2, 0) if dump else (tng, auc, 0, lmode, 2, 0)
        if ng not in TO_128:
            return None
        return (ng, 0, 1, LM_HBM, 2, 0) if dump else (ng, auc, 0, lmode, 2, spec)
    spec = 1 if spec == 1 and not dump else 0
    if ng in TO_64 + (16, 32, 64):
        tng = ng
    elif ng > 64 and ng % 8 == 0 and ng == ngt:
        tng = 0
    else:
        return None
    return (tng, 0, 1, LM_HBM, 2, 0) if dump else (tng, auc, 0, lmode, 2, spec)


def expected_ng(prec, k):
    ng = (k + 7) // 8
    have, chunk = ((TO_128 + (32, 64)), 16) if prec == "f32" else ((TO_64 + (16, 32, 64)), 8)
    for o in have:
        if ng <= o:
            return o
    return (ng + chunk - 1) // chunk * chunk


@pytest.fixture(scope="module")
def lib():
    from recometrics_amd import _binding
    return _binding.load()


@pytest.fixture(scope="module")
def rows(lib):
    out = {}
    for prec, eb in ELEM.items():
        n = lib.rm_debug_sweep_variants(eb, None, 0)
        buf = (ctypes.c_int * (6 * n))()
        assert lib.rm_debug_sweep_variants(eb, buf, n) == n
        out[prec] = [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]
    return out


def _find(lib, prec, req):
    out6 = (ctypes.c_int * 6)(*[-7] * 6)
    rc = lib.rm_debug_find_sweep(ELEM[prec], *req, out6)
    assert rc in (0, -1)
    return tuple(out6) if rc == 0 else None


@pytest.mark.parametrize("prec,count", [("f32", 272), ("f64", 143)])
def test_the_table_is_the_units_instantiations(rows, prec, count):
    want = [key for unit in expected_units()[prec].values() for key in unit]
    assert len(want) == len(set(want)) == count
    assert len(rows[prec]) == len(set(rows[prec])), "a variant is listed twice"
    assert set(rows[prec]) == set(want)
    assert len(rows[prec]) == count


def test_unknown_precision_is_refused(lib):
    assert lib.rm_debug_sweep_variants(2, None, 0) == -1
    assert lib.rm_debug_find_sweep(2, 8, 8, 0, 0, 0, 2, 0, None) == -1
    assert lib.rm_debug_supported_ng(2, 64) == -1


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_every_request_gets_the_variant_the_rules_give(lib, rows, prec):
    ngs = list(range(1, 21)) + [24, 32, 48, 64, 72, 80, 96, 128, 136]
    table, n_found = set(rows[prec]), 0
    for ng, dngt, auc, dump, lmode, nsub, spec in itertools.product(ngs, (0, 8), (0, 1), (0, 1), (0, 1, 2), (2, 3), (0, 1, 2)):
        req = (ng, ng + dngt, auc, dump, lmode, nsub, spec)
        got, want = _find(lib, prec, req), expected_key(prec, *req)
        assert got == want, (prec, req, got, want)
        if got is not None:
            n_found += 1
            assert got in table, (prec, req, got)
    assert n_found > 1000


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_every_factor_count_runs_on_a_group_count_that_has_kernels(lib, rows, prec):
    with_lists = {key[0] for key in rows[prec] if not key[2]}
    for k in range(1, 1101):
        ng = lib.rm_debug_supported_ng(ELEM[prec], k)
        assert ng == expected_ng(prec, k), (prec, k, ng)
        assert ng * 8 >= k
        for lmode in (LM_LDS, LM_HBM, LM_APPEND):       # the pipeline packs for ng groups and asks for them: ngt = ng
            key = _find(lib, prec, (ng, ng, 1, 0, lmode, 2, 0))
            assert key is not None and key[0] in with_lists and not key[2], (prec, k, ng, key)
            assert key[0] == (ng if ng <= 64 else 0)
