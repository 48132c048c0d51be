"""GPU: every row of the two tables of sweep-kernel instantiations (csrc/rm_sweep_units.hip) is executed once, and the library's
launch ledger (rm_debug_sweep_launched) proves which row each call ran.

The variants agree bit for bit by design, so a parity test that lands on another row than it meant passes all the same, and a
row nothing reaches is first executed by a user; every row is a compilation of its own (registers, spills, LDS carve-up).  The
visits are the data of tests/_sweep_plan.py -- one per row, checked against the table by tests/test_sweep_coverage_cpu.py -- and
the tests here are parametrised by translation unit.  Per metric visit: the switches, one cumulative call, the ledger (the
visit's row, no other list row, no dump row), every output against the oracle by check_request's rule (bit for bit; ROC-AUC
within an ulp: _util.roc_tol), and the lists -- hip.rank on the auc = 1 rows, recommend_topk on the auc = 0 rows, which must land on the same row.
Per dump visit: debug_scores against oracle.scores, and the ledger shows the dump row alone.

The problems are the smallest at which these kernels can still go wrong: 200 users (two user blocks in fp32, four in fp64, the
last block and its last group partial), 1,237 items (whole 64- and 96-item tiles and a ragged last one of either size), factor
counts with a ragged last group, two item ranges plus a tail level of three to merge, test rows of 1 to 63 items with a few
streamed users beyond and a few users without any."""
import ctypes
import functools

import numpy as np
import pytest

import _sweep_plan as plan
from _parity import NT
from _requests import TOPK8
from _util import assert_roc, assert_same_bits
from test_hip_recommend import check_lists, expected_lists
from test_sweep_table_cpu import ELEM

pytestmark = pytest.mark.gpu

M_USERS, N_ITEMS = 200, 1237
DTYPE = {"f32": np.float32, "f64": np.float64}
NO_TEST_USERS = (3, 77, 199)
LONG_ROWS = {10: 64, 60: 100, 130: 200, 150: 333, 198: 90}              # streamed users (more than 63 test items), in every user block


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


@pytest.fixture(scope="module")
def table(hip):
    out = {}
    for prec, eb in ELEM.items():
        n = hip.load().rm_debug_sweep_variants(eb, None, 0)
        buf = (ctypes.c_int * (6 * n))()
        assert hip.load().rm_debug_sweep_variants(eb, buf, n) == n
        out[prec] = [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]
    return out


def launched(hip, table, prec):
    """{row: launches since the reset}, rows that were launched"""
    n = len(table[prec])
    buf = (ctypes.c_int * n)()
    assert hip.load().rm_debug_sweep_launched(ELEM[prec], buf, n) == n
    return {table[prec][i]: buf[i] for i in range(n) if buf[i]}


def launched_anywhere(hip, table):
    return {(prec, key): c for prec in table for key, c in launched(hip, table, prec).items()}


@functools.lru_cache(maxsize=None)
def split():
    """train and test rows, the same for every factor count and precision"""
    rng = np.random.default_rng(20240)
    train, test, vals = [], [], []
    for u in range(M_USERS):
        n_test = 0 if u in NO_TEST_USERS else LONG_ROWS.get(u, 1 + (u * 37) % 63)       # 1 .. 63, every length
        items = rng.permutation(N_ITEMS)[:n_test + int(rng.integers(5, 60))]
        test.append(np.sort(items[:n_test]))
        train.append(np.sort(items[n_test:]))
        vals.append(rng.integers(1, 6, n_test))
    ptr = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    cat = lambda rows, dt: np.concatenate(rows).astype(dt)
    return (ptr(train), cat(train, np.int32)), (ptr(test), cat(test, np.int32), cat(vals, np.float64))


@functools.lru_cache(maxsize=None)
def problem(prec, factors):
    from recometrics_amd.synth import make_factors
    A, B = make_factors(M_USERS, N_ITEMS, factors, DTYPE[prec], seed=factors)
    train, (tep, tei, tev) = split()
    return dict(A=A, B=B, train=train, test=(tep, tei, tev.astype(DTYPE[prec])))


# the oracle's answers, once per (precision, factor count, K, request): auc, nsub and spec do not change them
@functools.lru_cache(maxsize=None)
def want_calc(oracle, prec, factors, K, request):
    pr = problem(prec, factors)
    return oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=request, cumulative=True, dtype=DTYPE[prec], nthreads=NT)


@functools.lru_cache(maxsize=None)
def want_rank(oracle, prec, factors, K):
    pr = problem(prec, factors)
    return oracle.rank(pr["A"], pr["B"], pr["train"], pr["test"], K, dtype=DTYPE[prec], nthreads=NT)


@functools.lru_cache(maxsize=None)
def want_lists(oracle, prec, factors, K):
    pr = problem(prec, factors)
    return expected_lists(oracle.scores(pr["A"], pr["B"], dtype=DTYPE[prec]), pr["train"], K)


@functools.lru_cache(maxsize=None)
def dump_problem(prec, factors):
    m, n = plan.DUMP_SHAPE[prec]
    rng = np.random.default_rng(7000 + factors)
    if prec == "f32":
        return rng.standard_normal((m, factors)).astype(np.float32), rng.standard_normal((n, factors)).astype(np.float32)
    return rng.standard_normal((m, factors)) * np.exp(rng.uniform(-20, 20, (m, 1))), rng.standard_normal((n, factors))


def set_switches(monkeypatch, env):
    for name in plan.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)                                  # (conftest.py: the library reads its switches again)


def metric_visit(hip, oracle, table, v, monkeypatch):
    from scipy.sparse import csr_array
    from recometrics_amd import recommend_topk
    from _parity import hip_calc
    dtype, pr = DTYPE[v.prec], problem(v.prec, v.factors)
    what = "%s %s %d factors K=%d %s -> row %s" % (v.prec, v.unit, v.factors, v.K, sorted(v.env.items()), v.key)
    auc = v.request == plan.ALL
    assert auc or v.request == TOPK8, what
    set_switches(monkeypatch, v.env)

    def ledger_shows_the_row(call):
        rows = launched_anywhere(hip, table)
        assert rows.get((v.prec, v.key), 0) >= 1, "%s: %s did not launch the row; launched %s" % (what, call, rows)
        others = {k: c for k, c in rows.items() if k != (v.prec, v.key)}
        assert not others, "%s: %s launched other rows as well: %s" % (what, call, others)     # list rows and dump rows alike

    hip.load().rm_debug_sweep_launched_reset()
    got = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], v.K, metrics=v.request, cumulative=True, dtype=dtype)
    ledger_shows_the_row("calc_metrics")
    want = want_calc(oracle, v.prec, v.factors, v.K, v.request)
    assert set(got) == set(want) and len(got) == len(v.request), what
    for name in want:
        if name == "ROC_AUC":
            assert_roc(got[name], want[name], dtype, what + ": " + name)
        else:
            assert_same_bits(got[name], want[name], what + ": " + name)

    trp, tri = pr["train"]
    if auc:
        tep, tei = pr["test"][:2]
        got_rank, w = hip.rank(pr["A"], pr["B"], trp, tri, tep, tei, v.K), want_rank(oracle, v.prec, v.factors, v.K)
        assert (got_rank["status"] == w["status"]).all(), what
        assert (got_rank["topk_idx"] == w["topk_idx"]).all(), what + ": top-K index lists differ"
        assert_same_bits(got_rank["topk_score"], w["topk_score"], what + ": top-K scores")
        assert (got_rank["pos_rank"] == w["pos_rank"]).all(), what + ": positive ranks differ"
    else:
        X = csr_array((np.ones(tri.shape[0], np.float32), tri, trp), shape=(M_USERS, N_ITEMS))
        hip.load().rm_debug_sweep_launched_reset()
        lists = recommend_topk(pr["A"], pr["B"], k=v.K, X_train=X)
        ledger_shows_the_row("recommend_topk")
        check_lists(lists, want_lists(oracle, v.prec, v.factors, v.K), what + ": recommend_topk")


def dump_visit(hip, oracle, table, v, monkeypatch):
    what = "%s %s dump at %d factors -> row %s" % (v.prec, v.unit, v.factors, v.key)
    set_switches(monkeypatch, v.env)
    A, B = dump_problem(v.prec, v.factors)
    hip.load().rm_debug_sweep_launched_reset()
    got = hip.debug_scores(A, B)
    rows = launched_anywhere(hip, table)
    assert set(rows) == {(v.prec, v.key)} and rows[(v.prec, v.key)] >= 1, "%s: launched %s" % (what, rows)
    assert_same_bits(got, oracle.scores(A, B, dtype=DTYPE[v.prec]), what)


@pytest.mark.parametrize("prec,unit", plan.unit_ids(), ids=["%s-%s" % pu for pu in plan.unit_ids()])
def test_every_row_of_the_unit_runs_and_is_the_row_that_ran(hip, oracle, table, prec, unit, monkeypatch):
    visits = plan.visits_of(prec, unit)
    assert visits
    for v in visits:
        assert v.key in table[prec], v
        (dump_visit if v.kind == "dump" else metric_visit)(hip, oracle, table, v, monkeypatch)


def test_the_problem_is_the_one_the_plan_assumes():
    """what _sweep_plan's restatement takes from the problem: tables of depth JMAX and no deeper, streamed users, users without
    test items, a train row for everybody, both tile sizes ragged"""
    (trp, _), (tep, _, _) = split()
    lengths = np.diff(tep)
    assert set(range(1, 64)) <= set(lengths.tolist()) and (lengths[list(NO_TEST_USERS)] == 0).all()
    assert sorted(lengths[lengths > 63].tolist()) == sorted(LONG_ROWS.values())
    assert (lengths[lengths <= 63].max() + 1) == 1 << plan.JMAX
    assert (np.diff(trp) > 0).all()
    assert M_USERS % 128 and M_USERS % 64 and M_USERS % 32 and M_USERS % 16 and N_ITEMS % 64 and N_ITEMS % 96
    padded = (N_ITEMS + 191) // 192 * 192                                # the dense train rows' stride: both ragged last tiles end inside it
    assert padded - 192 < N_ITEMS and (N_ITEMS + 63) // 64 * 64 <= padded and (N_ITEMS + 95) // 96 * 96 <= padded


def test_the_units_visited_are_the_whole_table(table):
    """computed from the plan and the table, not from what other tests left in the ledger"""
    for prec in table:
        asked = {v.key for p, unit in plan.unit_ids() if p == prec for v in plan.visits_of(prec, unit)}
        assert asked == set(table[prec]), (prec, sorted(set(table[prec]) - asked)[:8], sorted(asked - set(table[prec]))[:8])
    assert {prec: len(rows) for prec, rows in table.items()} == {"f32": 272, "f64": 143}
    assert plan.UNREACHABLE == []
