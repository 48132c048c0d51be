"""GPU: the ten metrics over candidate sets (rm_calc_metrics_candidates_* / k_metrics_candidates) against the oracle on the COMPLEMENT of
the candidate rows without noise and with cold start: every user, every output bit for bit (NaN masks included), ROC-AUC by assert_roc."""
import functools

import numpy as np
import pytest

import _layouts as lay
from _candidates import complement_of, csr_of, dup_run, rows_of, shuffled, spread_rows
from _util import assert_roc, assert_same_bits
from test_hip_entry_fields import dev  # noqa: F401 (a fixture)
from test_hip_recommend import hip  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
M, N = 300, 2600
ALL = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr")
REQUESTS = {"all": ALL, "default": ("p", "ap", "ndcg"), "hit_rr": ("hit", "rr"), "ndcg": ("ndcg",)}
WHOLE_ROW, NAN_ITEM, INF_ITEM = 20, 40, 41                           # users: test row = candidate row; lists the NaN / the +Inf item


def lengths(K):
    """entries per row: the edges of eligibility, of a wavefront's steps, of the two teams; everybody else above every K"""
    edges = sorted({0, 1, 2, K - 1, K, K + 1, 63, 64, 65, 255, 256, 257, 511, 2047, 2048} - {-1})
    return tuple(edges) + tuple(np.random.default_rng(1).integers(120, 400, M - len(edges)))


@functools.lru_cache(maxsize=None)
def problem(dtype, kf, K, structure="iid"):
    """A, B, candidate rows over items [0, N - 3) (the last three items are nobody's unless a structure lists them), test rows inside them"""
    from recometrics_amd.synth import make_factors
    A, B = (x.copy() for x in make_factors(M, N, kf, dtype, 7))
    rng = np.random.default_rng(2)
    rows = rows_of(spread_rows(lengths(K), N - 3, 3))
    if structure == "ties":                                           # runs of five equal scores, positives inside them; two users all +0
        B[:] = B[np.arange(N) // 5 * 5]
        A[30], A[31] = 0.0, -0.0
    if structure == "nonfinite":                                      # one NaN and one +Inf candidate score; a NaN item row nobody lists
        B[N - 1], B[N - 2], B[N - 3, 0] = np.nan, np.nan, np.inf
        rows[NAN_ITEM], rows[INF_ITEM] = np.append(rows[NAN_ITEM], N - 2), np.append(rows[INF_ITEM], N - 3)
    test = [np.sort(rng.choice(r[r < N - 3], min(1 + u % 12, (r < N - 3).sum()), replace=False)) for u, r in enumerate(rows)]
    test[WHOLE_ROW] = rows[WHOLE_ROW]
    tp, ti = csr_of(test)
    tv = (1 + rng.random(ti.shape[0])).astype(dtype)
    if structure == "values":                                         # a zero, a negative and a NaN test value (users with several test items)
        tv[tp[50]], tv[tp[51] + 1], tv[tp[52]], tv[tp[53]:tp[54]] = 0, -1, np.nan, -2
    return dict(A=A, B=B, cand=csr_of(rows), test=(tp, ti, tv))


@functools.lru_cache(maxsize=None)
def want_of(dtype, kf, K, structure, request, cumulative):
    """the oracle on the complement; at least 90 % of the users have finite outputs, so no case passes on NaN masks alone (the edge case:
    K = 1 without ROC-AUC, where the validity rule compares the first score with the K-th, itself, and every user is invalid)"""
    from oracle.oracle import Oracle
    P = problem(dtype, kf, K, structure)
    want = Oracle().calc(P["A"], P["B"], complement_of(P["cand"], N), P["test"], K, REQUESTS[request], cumulative, noise=False, cold=True, dtype=dtype)
    for name, w in want.items():
        assert np.isfinite(w.reshape(M, -1)).all(1).mean() >= (0.9 if K > 1 or "roc" in REQUESTS[request] else 0.0), name
    return want


def run(hip, dev, entry, P, K, request, cumulative, layout="D", outs_fill=7):
    """the requested metrics by the oracle's names, through the host or the device entry"""
    from oracle.oracle import NAMES
    A, B, (cp, ci), (tp, ti, tv) = P["A"], P["B"], P["cand"], P["test"]
    dtype, kf = A.dtype.type, A.shape[1]
    want = {name: name in REQUESTS[request] for name in ALL}
    if entry == "host":
        outs = hip.calc_metrics_candidates(A, kf, B, kf, cp, ci, tp, ti, tv, K, want, cumulative, 2, 1)
        return {NAMES[name]: o for name, o in zip(ALL, outs) if want[name]}
    at = []
    for X in (A, B):
        V, raw, off = lay.place_as(X, layout, lay.NAN_POISON[lay.PREC[np.dtype(dtype)]])
        at += [dev.put(raw) + off * raw.itemsize, V.strides[0] // raw.itemsize]
    shapes = [((M, K) if cumulative and i < 8 else (M,)) for i in range(10)]
    outs = [dev.put(np.full(s, outs_fill, dtype)) if want[name] else 0 for name, s in zip(ALL, shapes)]
    hip.calc_metrics_candidates_device(dtype, *at, M, N, kf, dev.put(cp), dev.put(ci), int(ci.shape[0]), dev.put(tp), dev.put(ti), dev.put(tv),
                                       int(ti.shape[0]), K, outs, cumulative=cumulative)
    return {NAMES[name]: dev.get(o, s, dtype) for name, o, s in zip(ALL, outs, shapes) if want[name]}


def check(got, want, dtype, what, roc_bitwise=False):
    assert set(got) == set(want), what
    for name in want:
        if name == "ROC_AUC" and not roc_bitwise:
            assert_roc(got[name], want[name], dtype, what)
        else:
            assert_same_bits(got[name], want[name], "%s: %s" % (what, name))


@pytest.mark.parametrize("cumulative", [False, True], ids=["single", "cumulative"])
@pytest.mark.parametrize("request_", list(REQUESTS))
@pytest.mark.parametrize("K", [1, 10, 100])
@pytest.mark.parametrize("entry", ["host", "dev"])
@DTYPES
def test_parity_with_the_oracle_on_the_complement(hip, dev, dtype, entry, K, request_, cumulative):
    got = run(hip, dev, entry, problem(dtype, 16, K), K, request_, cumulative)
    check(got, want_of(dtype, 16, K, "iid", request_, cumulative), dtype, "%s K=%d %s" % (entry, K, request_))


@pytest.mark.parametrize("kf", [1, 17, 130])
@DTYPES
def test_factor_counts_and_a_strided_unaligned_layout(hip, dev, dtype, kf):
    dense = run(hip, dev, "dev", problem(dtype, kf, 10), 10, "all", True)
    check(dense, want_of(dtype, kf, 10, "iid", "all", True), dtype, "%d factors" % kf)
    if kf == 17:
        check(run(hip, dev, "dev", problem(dtype, kf, 10), 10, "all", True, layout="RO"), dense, dtype, "layout RO", roc_bitwise=True)


@pytest.mark.parametrize("cumulative", [False, True], ids=["single", "cumulative"])
@pytest.mark.parametrize("structure", ["ties", "nonfinite", "values"])
@DTYPES
def test_structured_scores_and_test_values(hip, dev, dtype, structure, cumulative):
    want = want_of(dtype, 16, 10, structure, "all", cumulative)
    if structure == "values":                                         # deviation D6: a NaN among a user's test VALUES makes its NDCG NaN
        want = dict(want, **{"NDCG@K": want["NDCG@K"].copy()})        # (the oracle, as the reference, feeds it to std::partial_sort)
        want["NDCG@K"][52] = np.nan
    check(run(hip, dev, "dev", problem(dtype, 16, 10, structure), 10, "all", cumulative), want, dtype, structure)
    if structure == "ties":
        assert np.isnan(want["P@K"].reshape(M, -1)[30:32]).all()      # every score equal: invalid
    if structure == "nonfinite":
        assert np.isnan(want["PR_AUC"][[NAN_ITEM, INF_ITEM]]).all()


@DTYPES
def test_shuffled_rows_with_duplicates_equal_the_sorted_distinct_rows(hip, dev, dtype):
    P = problem(dtype, 16, 10)
    rows = [dup_run(r, 30, 70) if 100 <= len(r) < 1900 else r for r in rows_of(P["cand"])]      # one id 70 times, across entry 64
    rows = [np.sort(np.concatenate([r, r[::3]])) if 2 <= len(r) < 1300 else r for r in rows]
    assert max(len(r) for r in rows) == 2048
    messy = dict(P, cand=shuffled(csr_of(rows), 4))
    for entry in ("host", "dev"):
        check(run(hip, dev, entry, messy, 10, "all", True), run(hip, dev, entry, P, 10, "all", True), dtype, entry, roc_bitwise=True)


@DTYPES
def test_a_test_item_outside_the_row_and_a_row_too_long(hip, dev, dtype):
    P = problem(dtype, 16, 10)
    plain = run(hip, dev, "dev", P, 10, "all", True)
    tp, ti, tv = P["test"]
    ti = ti.copy()
    ti[tp[101] - 1] = N - 1                                           # user 100's last test item: nobody's candidate
    got = run(hip, dev, "dev", dict(P, test=(tp, ti, tv)), 10, "all", True)
    others = np.arange(M) != 100
    for name in plain:
        assert np.isnan(got[name][100]).all(), name
        assert_same_bits(got[name][others], plain[name][others], name)
    rows = rows_of(P["cand"])
    long_user = [len(r) for r in rows].index(2048)
    rows[long_user] = dup_run(rows[long_user], 1000, 2)               # 2,049 entries, 2,048 distinct
    for entry in ("host", "dev"):
        with pytest.raises(RuntimeError, match="candidate row %d has more than 2048 entries.*sweep" % long_user):
            run(hip, dev, entry, dict(P, cand=csr_of(rows)), 10, "all", True)
    # (the device entry's outputs stay as they were: the call is refused behind the plan stage, in front of the metric kernel)
    A, B, (cp, ci) = P["A"], P["B"], csr_of(rows)
    out = dev.put(np.full(M, 7, dtype))
    with pytest.raises(RuntimeError, match="candidate row"):
        hip.calc_metrics_candidates_device(dtype, dev.put(A), 16, dev.put(B), 16, M, N, 16, dev.put(cp), dev.put(ci), int(ci.shape[0]), dev.put(tp),
                                           dev.put(P["test"][1]), dev.put(tv), int(ti.shape[0]), 10, [out] + [0] * 9)
    assert (dev.get(out, (M,), dtype) == 7).all()


def test_batches_and_shards_equal_the_plain_call(hip, dev, monkeypatch):
    P = problem(F32, 16, 10)
    plain = run(hip, dev, "host", P, 10, "all", True)
    hip.set_devices([0, 0, 0])
    try:
        check(run(hip, dev, "host", P, 10, "all", True), plain, F32, "three shards", roc_bitwise=True)
    finally:
        hip.set_devices([])
    monkeypatch.setenv("RM_BATCH_USERS", "128")
    check(run(hip, dev, "host", P, 10, "all", True), plain, F32, "three batches", roc_bitwise=True)


@pytest.mark.parametrize("cumulative", [False, True], ids=["single", "cumulative"])
@DTYPES
def test_equals_the_metric_entry_on_the_complement(hip, dev, dtype, cumulative):
    from oracle.oracle import NAMES
    P, K = problem(dtype, 16, 10), 10
    train, test = complement_of(P["cand"], N), P["test"]
    shapes = [((M, K) if cumulative and i < 8 else (M,)) for i in range(10)]
    outs = [dev.put(np.full(s, 7, dtype)) for s in shapes]
    hip.calc_metrics_device(dtype, dev.put(P["A"]), 16, dev.put(P["B"]), 16, M, N, 16, dev.put(train[0]), dev.put(train[1]), int(train[1].shape[0]),
                            dev.put(test[0]), dev.put(test[1]), dev.put(test[2]), int(test[1].shape[0]), K, outs, cumulative=cumulative,
                            break_ties_with_noise=False, consider_cold_start=True)
    sweep = {NAMES[name]: dev.get(o, s, dtype) for name, o, s in zip(ALL, outs, shapes)}
    check(run(hip, dev, "dev", P, K, "all", cumulative), sweep, dtype, "rm_calc_metrics_dev_*", roc_bitwise=True)
