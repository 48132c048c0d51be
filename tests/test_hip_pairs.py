"""GPU: the pairwise plan of tests/_pairs_plan.py, one small call per case, against the oracle.

The suite's other GPU files vary one or two options of a metric call and hold the rest at their defaults.  Here every allowed pair
of levels of two options -- entry, precision, k_metrics regime, request, cumulative, tie noise, eligibility keywords, structure of the
scores, test items inside train rows, host batches, device list, item splits -- meets in at least one call (the plan's coverage is
tests/test_pairs_plan_cpu.py's to prove, with the conditions that keep a case from passing empty).

Per case: the environment levels and the device list are set, ONE call is made, and it is compared with oracle.calc under the same
keywords -- the set of returned outputs, every output bit for bit, ROC-AUC by assert_roc (tests/_util.py).  The score-matrix entry
gets S = oracle.scores(A, B) and must return what the factor call's oracle returns.  Where the library reports
a level, the test asserts that it took effect: the number of host batches of every user range in the library's own trace of the
host entry (RM_HOST_TRACE, on stderr), the item splits and the score entry's user count in rm_get_timings, the list mode of the
k_metrics regime in the sweep launch ledger.

RM_BATCH_USERS=64 meets the score-matrix entry only: from factors a batch holds whole 1,024s of users, so this family's 200 users
are one batch whatever the switch says (plan.EXCLUDED; the last test shows it on the device).  Host batches with the tie noise are
tests/test_hip_entry_fields.py's, tests/test_hip_multi.py's and tests/test_hip_requests.py's, at 2,500 users and more."""
import ctypes
import re

import numpy as np
import pytest

import _pairs as pairs
import _pairs_plan as plan
from _parity import hip_calc
from _util import assert_roc, assert_same_bits
from test_hip_scores import scores_calc
from test_sweep_table_cpu import ELEM, LM_APPEND, LM_LDS

pytestmark = pytest.mark.gpu
SWITCHES = ("RM_BATCH_USERS", "RM_DEBUG_SPLITS")
HOST_TRACE = re.compile(r"rm host trace \((\d+) batches")


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


@pytest.fixture
def device_list(hip):
    """the process's device list as the test found it, whatever the test did to it and however it ended"""
    before = hip.get_devices()
    yield
    hip.set_devices(before)


def launched_rows(hip, prec):
    """the sweep launch ledger since its reset: {(ng, auc, dump, lmode, nsub, spec): launches}"""
    lib = hip.load()
    n = lib.rm_debug_sweep_variants(ELEM[prec], None, 0)
    keys, counts = (ctypes.c_int * (6 * n))(), (ctypes.c_int * n)()
    assert lib.rm_debug_sweep_variants(ELEM[prec], keys, n) == n and lib.rm_debug_sweep_launched(ELEM[prec], counts, n) == n
    return {tuple(keys[6 * i:6 * i + 6]): counts[i] for i in range(n) if counts[i]}


def expected_list_mode(case):
    """fp32 at 20 factors runs three sub-tiles: its lists stay in LDS below k_metrics = 20 and go to the lane buffers from there on;
    fp64 takes the lane buffers at every k_metrics (csrc/rm_lib.hip lane_lists_possible; tests/_sweep_plan.py predict_choice)"""
    return LM_LDS if case.dtype == "f32" and case.K < 20 else LM_APPEND


@pytest.mark.parametrize("case", plan.CASES, ids=[plan.case_id(c) for c in plan.CASES])
def test_one_call_per_case_equals_the_oracle(hip, oracle, case, monkeypatch, device_list, capfd):
    pr, K, dtype, kw = pairs.problem_of(case), case.K, pairs.DTYPE[case.dtype], plan.call_kw(case)
    what = plan.case_id(case)
    req = plan.REQUESTS[case.request]
    want = pairs.want_of(oracle, case)                      # (the factor call's values for either entry)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in plan.env_of(case).items():
        monkeypatch.setenv(name, value)                     # (conftest.py: the library reads its switches again)
    hip.set_devices(plan.DEVICES[case.devices])
    assert hip.get_devices() == plan.DEVICES[case.devices]
    hip.load().rm_debug_sweep_launched_reset()
    monkeypatch.setenv("RM_HOST_TRACE", "1")                # (one line per user range on stderr; the call itself is the same)
    capfd.readouterr()
    if case.entry == "scores":
        assert not kw["noise"]
        opts = {k: v for k, v in kw.items() if k not in ("noise", "seed")}
        got = scores_calc(hip, pairs.scores(oracle, pr, dtype), pr["train"], pr["test"], K, dtype=dtype, **opts)
    else:
        got = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, dtype=dtype, **kw)
    trace = capfd.readouterr().err
    tm = hip.timings()
    rows = {prec: launched_rows(hip, prec) for prec in ELEM}

    # the outputs
    assert set(got) == set(want) and len(got) == len(req), what
    for name in want:
        assert got[name].shape == want[name].shape and got[name].dtype == dtype, (what, name)
        if name == "ROC_AUC":
            assert_roc(got[name], want[name], dtype, what + ": " + name)
        else:
            assert_same_bits(got[name], want[name], what + ": " + name)

    # the levels the library reports
    ev = pairs.evaluated(pr, K, **kw)
    ranges, cuts = plan.shard_ranges(pairs.M_USERS, len(plan.DEVICES[case.devices])), plan.cuts_of(case, pairs.M_USERS)
    assert sorted(int(b) for b in HOST_TRACE.findall(trace)) == sorted(len(c) - 1 for c in cuts), \
        "%s: batches per user range %s expected, the host entry traced: %s" % (what, [len(c) - 1 for c in cuts], trace[:300])
    assert (case.batches == "64") == any(len(c) > 2 for c in cuts), what
    other = "f64" if case.dtype == "f32" else "f32"
    assert not rows[other], "%s: kernels of the other precision ran: %s" % (what, rows[other])
    if case.entry == "scores":
        assert not rows[case.dtype], "%s: the score-matrix entry launched a sweep: %s" % (what, rows[case.dtype])
        users = tm["sweep_blocks"]                          # (out[6]: the evaluated users of the last batch of the first user range)
        last = slice(ranges[0][0] + cuts[0][-2], ranges[0][0] + cuts[0][-1])
        assert users == ev[last].sum(), "%s: %d users evaluated in the batch of users %d ... %d, %d expected" % (what, users, last.start, last.stop - 1, ev[last].sum())
    else:
        lists = {key: c for key, c in rows[case.dtype].items() if not key[2]}
        assert lists and len(lists) == len(rows[case.dtype]), "%s: launched %s" % (what, rows[case.dtype])
        auc = int(bool(set(req) & {"roc", "pr"}))
        assert any(key[1] == auc and key[3] == expected_list_mode(case) for key in lists), \
            "%s: no launch of list mode %d with auc = %d among %s" % (what, expected_list_mode(case), auc, lists)
        if case.splits == "3":
            assert tm["item_splits"] == 3, "%s: RM_DEBUG_SPLITS=3 gave %s item ranges" % (what, tm["item_splits"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_from_factors_the_200_users_are_one_batch_whatever_the_switch_says(hip, oracle, monkeypatch, capfd, dtype):
    """why the plan excludes (entry = factors, batches = 64): the factor entry raises RM_BATCH_USERS to whole 1,024s of users, its
    own trace speaks of ONE batch, and the outputs are the oracle's.  If this fails because the trace speaks of four, the library
    has learnt small batches: take the pair out of plan.EXCLUDED, and the noise and the item splits meet the batches in the plan."""
    pr, K = pairs.problem(dtype, 10, "iid", "none"), 10
    want = pairs.want(oracle, pr, K, dtype, metrics=plan.REQUESTS["all"])
    monkeypatch.delenv("RM_DEBUG_SPLITS", raising=False)
    monkeypatch.setenv("RM_BATCH_USERS", "64")
    monkeypatch.setenv("RM_HOST_TRACE", "1")
    capfd.readouterr()
    got = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, dtype=dtype, metrics=plan.REQUESTS["all"])
    trace = capfd.readouterr().err
    assert HOST_TRACE.findall(trace) == ["1"], trace[:300]
    assert set(got) == set(want)
    for name in want:
        if name == "ROC_AUC":
            assert_roc(got[name], want[name], dtype, name)
        else:
            assert_same_bits(got[name], want[name], name)
