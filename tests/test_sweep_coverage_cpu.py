"""CPU-only: the plan of tests/_sweep_plan.py against the table of sweep-kernel instantiations, and the launch ledger at rest.

tests/test_hip_sweep_rows.py executes the plan on a GPU; what can be said without one is said here: every row of both tables has
exactly one primary visit, no visit names a key outside the table, the key the plan predicts for a visit -- from its restatement
of the pipeline's choice of list scheme, sub-tile count and specialisation -- is the key the library's own rule gives for that
choice, and the ledger's exports count rows as the table does."""
import ctypes

import pytest

import _sweep_plan as plan
from test_sweep_table_cpu import ELEM, _find, expected_units, lib, rows  # noqa: F401  (fixtures)


@pytest.mark.parametrize("prec,count", [("f32", 272), ("f64", 143)])
def test_every_row_has_exactly_one_primary_visit(rows, prec, count):
    table = rows[prec]
    assert len(table) == len(set(table)) == count
    primary = [v.key for v in plan.VISITS if v.prec == prec and v.primary]
    twice = sorted({k for k in primary if primary.count(k) > 1})
    assert not twice, "rows with more than one primary visit: %s" % twice[:8]
    unreachable = {key for p, key, _ in plan.UNREACHABLE if p == prec}
    assert unreachable <= set(table)
    missing = sorted(set(table) - set(primary) - unreachable)
    assert not missing, "rows without a visit: %s" % missing[:8]
    outside = sorted({v.key for v in plan.VISITS if v.prec == prec} - set(table))
    assert not outside, "the plan names keys outside the table: %s" % outside[:8]
    assert not unreachable & set(primary)


def test_no_row_is_declared_unreachable():
    """(a row no entry point reaches is a finding: it is listed in the plan with the source line that proves it, and this test
    is where the list is seen to be empty)"""
    assert plan.UNREACHABLE == []


def test_a_visit_runs_in_the_unit_of_its_row():
    units = expected_units()
    for v in plan.VISITS:
        assert v.key in units[v.prec][v.unit], v
    assert sorted(plan.unit_ids()) == sorted((p, u) for p in units for u in units[p])
    assert len([u for p, u in plan.unit_ids() if p == "f32"]) == 11 and len([u for p, u in plan.unit_ids() if p == "f64"]) == 4


def test_the_library_gives_every_visit_the_key_the_plan_predicts(lib):
    for v in plan.VISITS:
        ng = lib.rm_debug_supported_ng(ELEM[v.prec], v.factors)
        assert ng == plan.supported_ng(v.prec, v.factors), v
        if v.kind == "dump":
            req = (ng, ng, 0, 1, plan.LM_HBM, 2, 0)
        else:
            auc = v.request == plan.ALL
            assert auc or v.request == plan.TOPK8, v
            png, lmode, nsub, spec = plan.predict_choice(v.prec, v.factors, v.K, auc, v.env)
            assert png == ng, v
            req = (ng, ng, int(auc), 0, lmode, nsub, spec)
        assert _find(lib, v.prec, req) == v.key, (v, req)


def test_second_visits_are_where_the_switches_are_read_at_run_time():
    """a second visit lands on a SPEC 0 row that has a primary visit of its own, under other switches"""
    second = [v for v in plan.VISITS if not v.primary]
    assert second
    primary = {(v.prec, v.key): v for v in plan.VISITS if v.primary}
    for v in second:
        assert v.key[5] == 0 and v.key[2] == 0, v
        assert (v.prec, v.key) in primary and primary[(v.prec, v.key)].env != v.env, v
    ext = {(v.prec, v.key) for v in second if "RM_DEBUG_EXT_TOPK" in v.env}
    assert ext == {(p, k) for (p, k) in primary if k[3] == plan.LM_APPEND and k[5] == 0 and not k[2]}
    csr = {(v.prec, v.key) for v in second if "RM_DEBUG_NO_TRAIN_BITS" in v.env}
    assert csr == {(p, k) for (p, k) in primary if p == "f32" and 0 < k[0] <= 16 and k[5] == 0 and not k[2]}


def test_the_plan_asks_only_for_switches_it_declares():
    for v in plan.VISITS:
        assert set(v.env) <= set(plan.SWITCHES), v
        if v.kind == "metric":
            assert v.env["RM_DEBUG_SPLITS"] == "2,1,3", v


@pytest.mark.parametrize("prec,count", [("f32", 272), ("f64", 143)])
def test_the_ledger_counts_rows_as_the_table_does(lib, prec, count):
    lib.rm_debug_sweep_launched_reset()
    assert lib.rm_debug_sweep_launched(ELEM[prec], None, 0) == count
    buf = (ctypes.c_int * (count + 1))(*[-7] * (count + 1))
    assert lib.rm_debug_sweep_launched(ELEM[prec], buf, count) == count
    assert list(buf[:count]) == [0] * count and buf[count] == -7          # nothing launched; nothing written behind `cap`
    short = (ctypes.c_int * 4)(*[-7] * 4)
    assert lib.rm_debug_sweep_launched(ELEM[prec], short, 3) == count and list(short) == [0, 0, 0, -7]


def test_the_ledger_refuses_an_unknown_precision(lib):
    assert lib.rm_debug_sweep_launched(2, None, 0) == -1
    buf = (ctypes.c_int * 2)(-7, -7)
    assert lib.rm_debug_sweep_launched(0, buf, 2) == -1 and list(buf) == [-7, -7]
