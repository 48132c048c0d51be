"""GPU: k_topk_candidates (csrc/rm_candidates.hpp) on rows that are not i.i.d.: scores ordered along the row, bounds inside runs of
exact ties, duplicates by the wavefront and by the step, non-finite scores far below an established bound, factor counts over several
steps in every pair of layouts, long rows next to a batch's or a shard's edge.

The reference everywhere: expected_lists(Oracle().scores(A, B), complement of the candidate rows, K) through check_lists -- every
user, ids, status, score bits; a user with a non-finite candidate score is compared too (status 2, ids -1, scores NaN).  The cases
are tests/_candidates.py's; tests/test_candidates_structured_cpu.py proves without a GPU that they reach the kernel's branches."""
import numpy as np
import pytest

import _candidates as cs
import _layouts as lay
from _candidates import F32, complement_of, rows_of, shuffled, want_of
from test_hip_candidates import run_dev, run_host
from test_hip_entry_fields import dev  # noqa: F401 (a fixture)
from test_hip_recommend import check_lists, hip  # noqa: F401 (hip: a fixture)

pytestmark = pytest.mark.gpu
NAME = {np.float32: "f32", np.float64: "f64"}


@pytest.mark.parametrize("K", cs.ORDER_K)
@pytest.mark.parametrize("kind,dtype,kf", cs.ORDER_CASES, ids=["%s-%s-k%d" % (kind, NAME[d], kf) for kind, d, kf in cs.ORDER_CASES])
def test_order_along_long_rows(hip, kind, dtype, kf, K):
    case = cs.order_case(kind, dtype, kf)
    A, B, cand = case["A"], case["B"], case["cand"]
    assert np.diff(cand[0]).tolist() == list(cs.ORDER_COUNTS) and A.shape == (cs.ORDER_M, kf) and B.shape == (cs.ORDER_N, kf)
    got = run_host(hip, A, B, cand, K)
    check_lists(got, want_of("order", K, kind, dtype, kf), "%s, K = %d" % (kind, K))
    if kind in ("ascending", "blocks"):
        excl = complement_of(cand, cs.ORDER_N)
        check_lists(got, hip.recommend(A, kf, B, kf, excl[0], excl[1], K), "rm_recommend_* on the complement")


@pytest.mark.parametrize("K", cs.DUP_K)
@pytest.mark.parametrize("dtype,kf", cs.DUP_CASES, ids=["%s-k%d" % (NAME[d], kf) for d, kf in cs.DUP_CASES])
def test_duplicates_at_scale(hip, dev, dtype, kf, K):
    case = cs.duplicate_case(dtype, kf)
    A, B, cand = case["A"], case["B"], case["cand"]
    want = want_of("duplicates", K, dtype, kf)                       # (from the distinct sets)
    assert want[2].tolist() == [1 if name == ("empty",) else 0 for name in case["names"]]
    one = case["names"].index(("one_id",))
    assert want[0][one, 0] == 1234 and (want[0][one, 1:] == -1).all()
    check_lists(run_host(hip, A, B, cand, K), want, "sorted rows, host entry")
    check_lists(run_dev(hip, dev, A, B, cand, K), want, "sorted rows, device entry")
    check_lists(run_host(hip, A, B, shuffled(cand, 5), K), want, "shuffled rows, host entry")


@pytest.mark.parametrize("K", cs.NF_K)
@pytest.mark.parametrize("order,dtype", cs.NF_CASES, ids=["%s-%s" % (o, NAME[d]) for o, d in cs.NF_CASES])
def test_non_finite_scores_in_long_rows(hip, order, dtype, K):
    case = cs.nonfinite_case(order, dtype)
    A, B, cand = case["A"], case["B"], case["cand"]
    want = want_of("nonfinite", K, order, dtype)
    hit = np.isin(np.arange(cs.NF_M), list(case["hit"]))
    assert (want[2] == np.where(hit, 2, 0)).all() and (want[0][hit] == -1).all() and np.isnan(want[1][hit]).all() and not hit.all()
    if case["overflow"]:
        u, item = case["overflow"]
        assert np.isfinite(A[u]).all() and np.isfinite(B[item]).all() and cs.scores_of("nonfinite", order, dtype)[u, item] == np.inf
    check_lists(run_host(hip, A, B, cand, K), want, "%s, K = %d" % (order, K))


def _vector_loads_with_a_partial_piece(dtype, kf):
    """(pad, off) of _layouts.place that rounds the stride up to 16 bytes behind a 16-byte aligned base: the kernel's vector loads
    are admitted (the named layout RA pads by a fixed 16 bytes, which keeps such a stride only where kf is a multiple already)"""
    ve = 16 // np.dtype(dtype).itemsize
    return ((-kf) % ve or ve, 0)


@pytest.mark.parametrize("dtype,kf", cs.COUNTS_CASES, ids=["%s-k%d" % (NAME[d], kf) for d, kf in cs.COUNTS_CASES])
def test_factor_counts_over_several_steps_in_every_layout(hip, dev, dtype, kf):
    case = cs.counts_case(dtype, kf)
    A, B, cand, K = case["A"], case["B"], case["cand"], cs.COUNTS_K
    dense = run_dev(hip, dev, A, B, cand, K)
    check_lists(dense, want_of("counts", K, dtype, kf), "dense, %d factors" % kf)
    assert ("RA", "RA") in lay.PAIRS and lay.CONTROL == ("D", "D")
    for la, lb in lay.PAIRS:
        check_lists(run_dev(hip, dev, A, B, cand, K, layout=la, layout_b=lb), dense, "A as %s, B as %s" % (la, lb))
    aligned = _vector_loads_with_a_partial_piece(dtype, kf)
    assert (kf + aligned[0]) * np.dtype(dtype).itemsize % 16 == 0
    check_lists(run_dev(hip, dev, A, B, cand, K, layout="RO", layout_b=aligned), dense, "A as RO, B with a stride rounded up to 16 bytes")
    check_lists(run_dev(hip, dev, A, B, cand, K, layout=aligned), dense, "both with a stride rounded up to 16 bytes")


def test_long_and_duplicate_rows_at_batch_and_shard_edges(hip, dev, monkeypatch):
    case = cs.edge_case()
    A, B, cand, K = case["A"], case["B"], case["cand"], cs.EDGE_K
    assert A.dtype == F32 and A.shape == (cs.EDGE_M, cs.EDGE_KF) and [rows_of(cand)[u].shape[0] for u in cs.EDGE_USERS] == [2305, 1199, 3000, 0, 2305, 1199, 3000]
    plain = run_dev(hip, dev, A, B, cand, K)
    check_lists(plain, want_of("edges", K), "device entry")
    hip.set_devices([0, 0, 0])
    try:
        check_lists(run_host(hip, A, B, cand, K), plain, "three shards")
    finally:
        hip.set_devices([])
    monkeypatch.setenv("RM_BATCH_USERS", "1024")
    try:
        check_lists(run_host(hip, A, B, cand, K), plain, "three batches")
    finally:
        monkeypatch.delenv("RM_BATCH_USERS")
