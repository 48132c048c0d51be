"""GPU: a context keeps what it derived from a call's train / test split and the next call on the same split runs on it.

The device-pointer entry with torch tensors as memory owners, in a process of its own per precision and per way of masking the
train items (dense train rows on / RM_DEBUG_NO_TRAIN_BITS): tests/_split_cache_child.py plays the scenarios below and compares every
output array of every call, bit for bit, with the same call made with RM_DEBUG_NO_SPLIT_CACHE=1 on freshly allocated arrays.
300 users x 700 items x 16 factors, make_interactions with a mean of 120 interactions per user, half of every row held out: table
users of every depth, users with more than 63 test items (streamed), and a few users without a train or a test row.  `split_reused` (rm_get_timings) says which calls ran on the kept split.

What is kept is only ever used for plain metric calls by device pointers (tie noise off, all users): the other calls answer -1."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _parity import NT, _check_against_oracle
from _util import assert_roc, assert_same_bits
from test_hip_parity import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = [("f32", True), ("f32", False), ("f64", True), ("f64", False)]
IDS = ["%s-%s" % (p, "dense_rows" if d else "no_train_bits") for p, d in CONFIGS]


@functools.lru_cache(maxsize=None)
def _played(prec, dense):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RM_")}
    if not dense:
        env["RM_DEBUG_NO_TRAIN_BITS"] = "1"
    res = subprocess.run([sys.executable, os.path.join(HERE, "_split_cache_child.py"), prec], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("prec,dense", CONFIGS, ids=IDS)
def test_three_models_on_one_split(hip, oracle, prec, dense, monkeypatch):
    got = _played(prec, dense)
    assert got["yardstick_errors"].keys() == {"('index_n', 2)"}, got["yardstick_errors"]
    assert got["three_calls"] == {"reused": [0, 1, 1], "equal": [True, True, True]}, got["three_calls"]
    # the same problem against the oracle (host entry), under the same switches
    from recometrics_amd.synth import make_factors
    from _split_cache_child import split_arrays
    dtype = np.float32 if prec == "f32" else np.float64
    if not dense:
        monkeypatch.setenv("RM_DEBUG_NO_TRAIN_BITS", "1")
    A, B = make_factors(300, 700, 16, dtype, seed=100)
    trp, tri, tep, tei, tev = split_arrays(dtype)
    npos = np.diff(tep)
    assert (npos > 63).any() and all(((npos > (1 << j) - 1) & (npos <= (2 << j) - 1)).any() for j in range(1, 6)), "streamed users and table users of every depth from 1"
    assert (npos == 0).any() and (np.diff(trp) == 0).any()
    _check_against_oracle(hip, oracle, {"A": A, "B": B, "train": (trp, tri), "test": (tep, tei, tev)}, 10, dtype=dtype)
    # _check_against_oracle goes through the host-pointer entry, which never reuses a split: the outputs of the third device call above,
    # which ran on the kept split (another model: seed 102), against the oracle as well -- bitwise but for ROC-AUC, as in _parity
    from oracle.oracle import NAMES
    A2, B2 = make_factors(300, 700, 16, dtype, seed=102)
    want = oracle.calc(A2, B2, (trp, tri), (tep, tei, tev), 10, cumulative=False, dtype=dtype, nthreads=NT)
    for name, values in zip(hip.METRIC_ORDER, got["reused_outputs"]):
        mine = np.asarray(values, dtype=np.float64).astype(dtype)
        if NAMES[name] == "ROC_AUC":
            assert_roc(mine, want[NAMES[name]], dtype, "reused call, %s" % name)
        else:
            assert_same_bits(mine, want[NAMES[name]], "reused call, %s (bitwise)" % name)


@pytest.mark.parametrize("prec,dense", CONFIGS, ids=IDS)
@pytest.mark.parametrize("what", ["a_test_item", "b_test_value", "c_train_index", "d_test_p", "e_train_p", "f_last_word"])
def test_contents_changed_in_place_are_noticed(prec, dense, what):
    """same pointers, same sizes, one element different: (a) a test item's id, its row still sorted, (b) a test value, (c) a train
    index, (d) / (e) an index pointer of the test / train matrix moved by one, so that one entry changes its owner, (f) the last
    element of an index array whose length is no multiple of four (behind the last 16-byte piece of the comparison)"""
    got = _played(prec, dense)["changed"][what]
    assert got["warm_reused"] == [0, 1] and got["warm_equal"] == [True, True], got
    assert got["reused"] == 0 and got["equal"], got


@pytest.mark.parametrize("prec,dense", CONFIGS, ids=IDS)
@pytest.mark.parametrize("what", ["a_test_item", "c_train_index", "f_last_word"])
def test_index_arrays_that_are_not_16_byte_aligned(prec, dense, what):
    """the caller's four index arrays 4 bytes behind an allocation: the comparison's word-by-word path reuses equal contents and
    notices a changed element"""
    got = _played(prec, dense)["unaligned"][what]
    assert got["warm_reused"] == [0, 1] and got["warm_equal"] == [True, True], got
    assert got["reused"] == 0 and got["equal"], got


@pytest.mark.parametrize("prec,dense", CONFIGS, ids=IDS)
def test_contents_made_invalid_in_place_are_validated_again(prec, dense):
    """after a call that reused the split: an index equal to n (the uncached call's error, word for word) and a descending pair
    inside a row (the uncached call's result: the library sorts a copy)"""
    got = _played(prec, dense)
    bad = got["invalid"]["index_n"]
    assert bad["warm_reused"] == [0, 1] and bad["equal"], bad
    assert "out of range" in bad["error"] and "row 123" in bad["error"], bad
    desc = got["invalid"]["descending"]
    assert desc["warm_reused"] == [0, 1] and desc["equal"] and desc["reused"] == 0 and desc["error"] is None, desc
    assert got["after_invalid"]


@pytest.mark.parametrize("prec,dense", CONFIGS, ids=IDS)
def test_the_request_changes_between_calls(prec, dense):
    """k_metrics, the metrics asked for (with and without ROC / PR-AUC), cumulative, the tie noise on and off, the precision"""
    for step in _played(prec, dense)["options"]:
        assert step["equal"] == [True, True], step
        assert step["reused"] == ([-1, -1] if step["kw"].get("noise") else [0, 1]), step


@pytest.mark.parametrize("prec,dense", CONFIGS, ids=IDS)
def test_released_workspace_and_other_entries_between_calls(prec, dense):
    got = _played(prec, dense)
    assert got["release"] == {"reused": [0, 0, 1], "equal": [True, True, True]}, got["release"]
    # lists (rm_recommend_dev_*) and metrics from a score matrix between metric calls: each plans for itself and voids what was kept
    assert got["between"] == {"reused": [0, 0, 0, 1], "equal": [True] * 6}, got["between"]
