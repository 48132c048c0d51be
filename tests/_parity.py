"""What the GPU parity tests share: the call through the C-ABI, the compiled reference as the second checker, and the whole
comparison of one problem with the oracle (status, top-K lists, positive ranks, every metric)."""
import os

import numpy as np

from _util import assert_close, assert_roc, assert_same_bits
from _util import same_bits as _util_same_bits
from oracle.ties import tie_pairs_per_user

TOL = 1e-5
NT = max(1, min(64, os.cpu_count() or 1))      # host threads for the oracle (the GPU box has many cores)


def hip_calc(hip, A, B, train, test, k, metrics=("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr"),
             cumulative=False, noise=False, cold=True, min_items_pool=2, min_pos_test=1, seed=1, dtype=np.float32, **_):
    from oracle.oracle import NAMES
    A = np.ascontiguousarray(A, dtype=dtype)
    B = np.ascontiguousarray(B, dtype=dtype)
    trp, tri = [np.ascontiguousarray(x, dtype=np.int32) for x in train[:2]]
    tep, tei = [np.ascontiguousarray(x, dtype=np.int32) for x in test[:2]]
    tev = np.ascontiguousarray(test[2], dtype=dtype) if len(test) > 2 and test[2] is not None else np.ones(tei.shape[0], dtype)
    want = {name: (name in metrics) for name in hip.METRIC_ORDER}
    outs = hip.calc_metrics(A, A.shape[1], B, B.shape[1], trp, tri, tep, tei, tev, k, want, cumulative, noise, cold,
                            min_items_pool, min_pos_test, 1, seed)
    return {NAMES[name]: arr for name, arr in zip(hip.METRIC_ORDER, outs) if want[name]}


_REF = []


def _reference():
    """the real reference as a second checker, when its compiled library is present (it is on the GPU box: oracle/_ref travels)"""
    if not _REF:
        from oracle.oracle import Reference, reference_available
        _REF.append(Reference() if reference_available() else None)
    return _REF[0]


def _check_against_oracle(hip, oracle, pr, k, dtype=np.float32, reference=True, **kw):
    want_rank = oracle.rank(pr["A"], pr["B"], pr["train"], pr["test"], k, dtype=dtype, nthreads=NT)
    trp, tri = pr["train"]
    tep, tei = pr["test"][:2]
    got_rank = hip.rank(np.ascontiguousarray(pr["A"], dtype), np.ascontiguousarray(pr["B"], dtype), trp, tri, tep, tei, k)
    assert (got_rank["status"] == want_rank["status"]).all()
    assert (got_rank["topk_idx"] == want_rank["topk_idx"]).all(), "top-K index lists differ"
    assert_same_bits(got_rank["topk_score"], want_rank["topk_score"], "top-K scores")
    assert (got_rank["pos_rank"] == want_rank["pos_rank"]).all(), "positive ranks differ"
    ref = _reference() if reference else None      # (False: inputs on which the reference's order of exact ties is not defined)
    for cumulative in (False, True):
        want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], k, cumulative=cumulative, dtype=dtype, nthreads=NT, **kw)
        got = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], k, cumulative=cumulative, dtype=dtype, **kw)
        if ref is not None:
            # not only the restatement: the REAL reference (oracle/_ref, compiled from /root/reference by oracle/Makefile; the
            # library travels to the GPU box) on the same inputs.  Noise off: exact ties are ordered by item id here and by
            # libstdc++'s sort there (deviation D4) -- the synthetic factors have none.
            real = ref.calc(pr["A"], pr["B"], pr["train"], pr["test"], k, cumulative=cumulative, dtype=dtype, nthreads=NT, **kw)
            # Noise off: scores that are EXACTLY equal (with 40,000 fp32 scores per user a handful of pairs always are) are ordered
            # by item id here and in the restatement, and by libstdc++'s introsort in the reference -- deviation D4.  Such a pair
            # changes a metric only when one of the two is a test item of the user (oracle/ties.py), so: EVERY user that differs
            # from the compiled reference -- in the last bit of any metric, or by more than 1e-5 in ROC-AUC (formed in x87 long
            # double there: an ulp apart for everybody) -- must have a candidate whose score equals one of its positives' scores
            # exactly, or the test fails.  A tied pair moves a positive by one rank, 1 / (positives x negatives) of ROC-AUC.
            n_users = len(tep) - 1
            differing = np.zeros(n_users, bool)
            for name in real:
                assert (np.isnan(got[name]) == np.isnan(real[name])).all(), name
                if name != "ROC_AUC":
                    assert_close(got[name], real[name], TOL, "%s cumulative=%s vs the compiled reference" % (name, cumulative))
                    diff = ~_util_same_bits(got[name], real[name]).reshape(n_users, -1).all(axis=1)
                    if name == "PR_AUC" and os.environ.get("RM_STREAM_BUDGET_MB") == "0":
                        diff &= np.diff(tep) <= 63          # deviation D7 (fallback only): per-chunk partial sums, a few ulp(fp64), checked below at 1e-12
                    differing |= diff
            d_roc = np.zeros(n_users)
            if "ROC_AUC" in real:
                r64 = np.nan_to_num(real["ROC_AUC"].astype(np.float64))
                d_roc = np.abs(np.nan_to_num(got["ROC_AUC"].astype(np.float64)) - r64) / np.maximum(1.0, np.abs(r64))   # (relative beyond magnitude 1, see assert_close)
                differing |= d_roc > TOL
            pairs = np.zeros(n_users, np.int64)
            if differing.any():
                who = np.flatnonzero(differing)
                sc = hip.debug_scores(np.ascontiguousarray(pr["A"][who], dtype), np.ascontiguousarray(pr["B"], dtype))
                noisy = bool(kw.get("noise"))
                pairs[who] = tie_pairs_per_user(sc, pr["train"], pr["test"], who, noise_zone=(2.0 ** -14 if noisy and dtype == np.float32 else None))
                unexplained = who[pairs[who] == 0]
                assert unexplained.size == 0, "users %s differ from the compiled reference without an exact tie on a positive" % unexplained[:8].tolist()
            npos_u = np.diff(tep).astype(np.float64)
            nneg_u = np.maximum(pr["B"].shape[0] - np.diff(trp) - npos_u, 1)
            assert (d_roc <= TOL + pairs / np.maximum(npos_u * nneg_u, 1)).all(), "ROC_AUC vs the compiled reference: %g" % d_roc.max()
        # PR_AUC of a user with more than 63 test items is assembled from per-chunk partial sums (finalize):
        # same terms, different association than the reference's single running sum -> a few ulp(fp64), checked at 1e-12
        # (only when such users take one sweep slot per chunk, RM_STREAM_BUDGET_MB=0; by default their ranks come from
        # their stored score rows and the sum is the reference's own left-to-right one: bitwise for every user)
        one_chunk = (np.diff(tep) <= 63) if os.environ.get("RM_STREAM_BUDGET_MB") == "0" else np.ones(len(tep) - 1, bool)
        for name in want:
            if name == "ROC_AUC":                          # (fp64 here, x87 long double there: an ulp of the output type, _util.roc_tol)
                assert_roc(got[name], want[name], dtype, "%s cumulative=%s" % (name, cumulative))
                continue
            assert_close(got[name], want[name], TOL, "%s cumulative=%s" % (name, cumulative))
            if name == "PR_AUC":
                assert_same_bits(got[name][one_chunk], want[name][one_chunk], "%s single-chunk users (bitwise)" % name)
                assert_close(got[name][~one_chunk], want[name][~one_chunk], 1e-12, "%s multi-chunk users" % name)
            else:
                assert_same_bits(got[name], want[name], "%s cumulative=%s (bitwise)" % (name, cumulative))
