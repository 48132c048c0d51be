"""CPU-only: what the C-ABI's metric / list entries answer to bad arguments, replayed from tests/golden/api/entry_errors.json.

The table (tests/golden/make_entry_errors.py) holds, for the sixteen entries and rm_rank_* in both precisions, every applicable defect
alone and every pair of two: the return code and the exact rm_last_error() text -- so also WHICH message a caller gets when two things
are wrong.  Every case is decided before a device is asked for, and no output array is written."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_entry_errors", os.path.join(GOLDEN, "make_entry_errors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "api", "entry_errors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from recometrics_amd import build as rb
    rb.build()
    from recometrics_amd import _binding
    return _binding.load()


def test_the_table_covers_every_entry(gen, table):
    assert set(table["cases"]) == {e + "_" + s for e in gen.FAMILIES for s in gen.SUFFIXES}
    assert sum(len(rows) for rows in table["cases"].values()) >= 400
    for entry in gen.FAMILIES:
        known = {" + ".join(c) for c in gen.cases_of(entry)}
        for suffix in gen.SUFFIXES:
            rows = table["cases"][entry + "_" + suffix]
            assert rows and set(rows) <= known, entry


@pytest.mark.parametrize("suffix", ["f32", "f64"])
@pytest.mark.parametrize("entry", ["rm_calc_metrics", "rm_calc_metrics_dev", "rm_rank", "rm_calc_metrics_scores", "rm_calc_metrics_scores_dev",
                                   "rm_recommend", "rm_recommend_dev", "rm_recommend_scores", "rm_recommend_scores_dev"])
def test_code_and_text_of_every_recorded_case(gen, table, lib, entry, suffix):
    for case, (want_rc, msg_index) in table["cases"][entry + "_" + suffix].items():
        rc, msg, outs = gen.call(lib, entry, suffix, case.split(" + "))
        assert (rc, msg) == (want_rc, table["messages"][msg_index]), (entry, suffix, case)
        for o in outs:
            assert (o == gen.SENTINEL).all(), (entry, suffix, case, "an output array was written")
