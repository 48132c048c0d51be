"""CPU-only: what the four public functions do with their arguments before the library is touched, replayed from
tests/golden/api/python_errors.json.

The table (tests/golden/make_python_errors.py) holds, for calc_reco_metrics, calc_reco_metrics_from_scores, recommend_topk and
recommend_topk_from_scores, one small valid call changed by every defect and input variant alone and by every pair of two: the
exception's type and exact text -- so also WHICH message a caller gets when two things are wrong, and whether it is an AssertionError
or a ValueError --, the warnings, what reached the binding (names, dtypes, shapes, strides, contents) and what came back.  The library
is not loaded: the host wrappers are replaced by the generator's recorder."""
import importlib.util
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUNCTIONS = ["calc_reco_metrics", "calc_reco_metrics_from_scores", "recommend_topk", "recommend_topk_from_scores"]


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_python_errors", os.path.join(GOLDEN, "make_python_errors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "api", "python_errors.json")) as f:
        return json.load(f)


def test_the_table_covers_every_case(gen, table):
    assert list(gen.FUNCTIONS) == FUNCTIONS and set(table["cases"]) == set(FUNCTIONS)
    for function in FUNCTIONS:
        cases = set(gen.cases_of(function))
        changes = gen.changes_of(function)
        assert () in cases and all((a,) in cases for a in changes), function
        for a, b in itertools.combinations(changes, 2):          # a pair is missing only by the rules of the generator's docstring
            same_argument = bool(set(changes[a][0]) & set(changes[b][0]))
            allocates = function == "calc_reco_metrics" and {a, b} == {"X_test 2^31-1 rows", "item_biases alone"}
            assert ((a, b) in cases) == (not same_argument and not allocates), (function, a, b)
        assert len(table["cases"][function]) == len(cases) and set(gen.decode(table, function)) == {" + ".join(c) for c in cases}, function


@pytest.mark.parametrize("function", FUNCTIONS)
def test_every_recorded_case(gen, table, function):
    from recometrics_amd import _binding
    before = {name: getattr(_binding, name) for name in list(gen.FUNCTIONS.values()) + ["has_openmp"]}
    got = json.loads(json.dumps(gen.records_of(function)))
    assert before == {name: getattr(_binding, name) for name in before}, "the recorder was left in place"
    recorded = gen.decode(table, function)
    assert list(recorded) == list(got)
    for label, rec in recorded.items():
        assert got[label] == rec, (function, label)


def test_the_file_is_what_the_generator_writes(gen, table, tmp_path):
    """the stated layout, so that running the generator again reproduces the committed file byte for byte"""
    gen.dump(table, str(tmp_path / "again.json"))
    assert (tmp_path / "again.json").read_bytes() == open(os.path.join(GOLDEN, "api", "python_errors.json"), "rb").read()
