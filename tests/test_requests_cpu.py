"""CPU-only: the problems of tests/_requests.py do what tests/test_hip_requests.py needs them to do -- asserted on the oracle's
outputs -- and the oracle agrees with the compiled reference under every request at these shapes (where oracle/_ref is built).

The rules a request without ROC-AUC changes (oracle/recometrics_oracle.cpp `eval_user`): who is evaluated at all, the partial
validity rule (best score == K-th score), and -- on the device -- where the tie noise's exact pass gets its users from.  On i.i.d.
factors none of them decides anybody's outputs; each builder below makes one of them decide at least a third of the users'."""
import inspect

import numpy as np
import pytest

from _requests import (ALL, COLD_USER, DEFAULT, F32, F64, LONG_ROWS, NT, ONLY_NDCG_USER, REQUESTS, TIE_REQUESTS, TOPK8, edge_problem,
                       equal_problem, long_rows_problem, oracle_against_reference, per_user, runs_problem, tie_problem, user_is_nan)
from _util import same_bits

EDGE_K = (1, 10, 100)
SEEDS = (2 ** 33 + 5, 1)


def calc(oracle, pr, K, dtype, req, **kw):
    return oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, dtype=dtype, nthreads=NT, **kw)


def nan_of(out, u):
    return {name: bool(np.isnan(arr[u]).all()) for name, arr in out.items()}


def test_the_requests_are_spelled_as_the_binding_spells_them():
    from recometrics_amd import _binding, calc_reco_metrics
    assert ALL == tuple(_binding.METRIC_ORDER)
    assert all(set(req) <= set(ALL) and len(set(req)) == len(req) for req in REQUESTS)
    assert TOPK8 == ALL[:8] and set(TIE_REQUESTS) <= set(REQUESTS)
    # DEFAULT is the call with every keyword at its default: precision, average precision, NDCG, tie noise on
    par = inspect.signature(calc_reco_metrics).parameters
    flags = dict(p="precision", tp="trunc_precision", r="recall", ap="average_precision", tap="trunc_average_precision", ndcg="ndcg",
                 hit="hit", rr="rr", roc="roc_auc", pr="pr_auc")
    assert tuple(nm for nm in ALL if par[flags[nm]].default) == DEFAULT
    assert par["break_ties_with_noise"].default is True and par["all_metrics"].default is False


# ---- 1. eligibility by request ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", EDGE_K)
def test_the_edge_users_are_planted(dtype, K):
    pr = edge_problem(dtype, K)
    ntr, nte = np.diff(pr["train"][0]), np.diff(pr["test"][0])
    assert list(nte[:6]) == [0, 1, 63, 64, 500, 500] and ntr[6] == 1000
    assert list(1000 - ntr[7:11]) == [1, max(1, K - 1), K, K + 1]
    u = ONLY_NDCG_USER
    tr = pr["train"][1][pr["train"][0][u]:pr["train"][0][u + 1]]
    te = pr["test"][1][pr["test"][0][u]:pr["test"][0][u + 1]]
    assert te.shape[0] == 40 and np.intersect1d(tr, te).size == 0 and np.union1d(tr, te).size == 1000
    assert ntr[COLD_USER] == 0 and nte[COLD_USER] > 0
    tev = pr["test"][2]
    assert (tev[pr["test"][0][13]:pr["test"][0][14]] == 0).all() and (tev[pr["test"][0][12]:pr["test"][0][13]] < 0).any()
    cold = edge_problem(dtype, K, cold_rows=True)
    assert (np.diff(cold["train"][0])[[20, 21, 22]] == 0).all() and (np.diff(cold["test"][0])[[20, 21, 22]] > 0).all()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_who_is_evaluated_depends_on_the_request(oracle, dtype):
    """K = 10, noise off, users 8 (C = K - 1), 9 (C = K), 13 (all-zero test values), 14 (train + test = catalogue), 15 (cold)"""
    K = 10
    pr = edge_problem(dtype, K)
    out = {req: calc(oracle, pr, K, dtype, req) for req in REQUESTS}
    for req in REQUESTS:
        assert all(nan_of(out[req], 8).values()), "C = K - 1 is invalid under %s" % (req,)
        assert not any(nan_of(out[req], COLD_USER).values()), "the cold user is evaluated under %s" % (req,)
        u13 = nan_of(out[req], 13)
        assert [nm for nm, isnan in u13.items() if isnan] == (["NDCG@K"] if "ndcg" in req else []), (req, u13)
    # C = K: alive through AP / TAP / RR / PR / ROC; P, TP, R, Hit are NaN whoever keeps it alive; NDCG is valid only beside them
    u9 = {req: nan_of(out[req], 9) for req in REQUESTS}
    assert u9[DEFAULT] == {"P@K": True, "AP@K": False, "NDCG@K": False}
    assert u9[TOPK8] == {"P@K": True, "TP@K": True, "R@K": True, "AP@K": False, "TAP@K": False, "NDCG@K": False, "Hit@K": True, "RR@K": False}
    assert u9[("ndcg",)] == {"NDCG@K": True} and u9[("p", "ndcg")] == {"P@K": True, "NDCG@K": True}
    assert u9[("p",)] == {"P@K": True} and u9[("tp", "r")] == {"TP@K": True, "R@K": True}
    assert u9[("hit", "rr")] == {"Hit@K": True, "RR@K": False} and u9[("ap", "tap")] == {"AP@K": False, "TAP@K": False}
    assert u9[("pr",)] == {"PR_AUC": False} and u9[("p", "pr")] == {"P@K": True, "PR_AUC": False}
    assert u9[("p", "roc")] == {"P@K": True, "ROC_AUC": False}
    # train + test = catalogue: alive only for NDCG, and then NDCG alone is valid
    u14 = {req: nan_of(out[req], ONLY_NDCG_USER) for req in REQUESTS}
    assert u14[("ndcg",)] == {"NDCG@K": False} and u14[("p",)] == {"P@K": True}
    assert u14[("p", "ndcg")] == {"P@K": True, "NDCG@K": False} and u14[DEFAULT] == {"P@K": True, "AP@K": True, "NDCG@K": False}
    for req in REQUESTS:
        if "ndcg" not in req:
            assert all(u14[req].values()), req


def test_which_requests_the_edge_users_tell_from_the_all_ten_call(oracle):
    """Per planted user, the NaN pattern of a request's outputs against the same outputs of the all-ten call.  ("p", "roc") never
    differs (ROC-AUC keeps every rule as the all-ten call has it): tests/test_hip_requests.py leaves it out of this section.  Every
    other request differs somewhere; at K = 1 for everybody -- the best score IS the K-th, so without ROC-AUC and without noise the
    partial rule holds nobody valid."""
    differs = {req: [] for req in REQUESTS}
    for K in EDGE_K:
        pr = edge_problem(F32, K)
        full = calc(oracle, pr, K, F32, ALL)
        for req in REQUESTS:
            out = calc(oracle, pr, K, F32, req)
            who = [u for u in range(16) if any(np.isnan(out[nm][u]) != np.isnan(full[nm][u]) for nm in out)]
            differs[req].append(who)
            if K == 1 and "roc" not in req:
                assert user_is_nan(out).all()
                assert np.isfinite(full["RR@K"]).sum() > 100
    assert differs[("p", "roc")] == [[], [], []]
    for req in REQUESTS:
        if req != ("p", "roc"):
            assert any(differs[req]), req
    assert differs[("ndcg",)][1] == [9] and differs[("p", "ndcg")][1:] == [[9], [9]]


# ---- 2. the partial validity rule -----------------------------------------------------------------------------------------------
TIE_K = (3, 10, 12, 20, 33, 50, 100, 300)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", TIE_K)
def test_tied_zeros_at_the_top_are_invalid_without_roc_auc_only(oracle, dtype, K):
    pr = tie_problem(dtype)
    contrast = calc(oracle, pr, K, dtype, ("p", "roc"))
    assert np.isfinite(contrast["P@K"]).all() and np.isfinite(contrast["ROC_AUC"]).all()
    who = None
    for req in TIE_REQUESTS:
        if "roc" in req:
            continue
        dead = user_is_nan(calc(oracle, pr, K, dtype, req))
        assert dead.sum() >= 100 and dead[::3].all(), (req, int(dead.sum()))
        assert who is None or (dead == who).all()
        who = dead
    assert who.sum() < 150                      # (the others stay valid: it is the rule, not the problem, that is NaN)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_runs_of_equal_scores_inside_and_beyond_k(oracle, dtype):
    pr = runs_problem(dtype)
    S = oracle.scores(pr["A"][:1], pr["B"], dtype=dtype)[0]
    top_run = int((S == S.max()).sum())
    assert 10 < top_run < 100 and (np.diff(S) >= 0).all() and (np.diff(S) == 0).mean() > 0.95
    for req in TIE_REQUESTS:
        dead10 = user_is_nan(calc(oracle, pr, 10, dtype, req))
        dead100 = user_is_nan(calc(oracle, pr, 100, dtype, req))
        assert not dead100.any(), req
        assert (not dead10.any()) if "roc" in req else dead10.sum() >= 100, (req, int(dead10.sum()))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_all_scores_equal_is_invalid_under_every_request(oracle, dtype):
    pr = equal_problem(dtype)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    assert (S == S[:, :1]).all()
    for req in TIE_REQUESTS:
        assert user_is_nan(calc(oracle, pr, 10, dtype, req)).all(), req
    assert user_is_nan(calc(oracle, pr, 10, dtype, DEFAULT, noise=True, seed=3)).all()


# ---- 3. tie noise without the AUCs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [10, 100, 300])
def test_the_noise_decides_a_third_of_the_users(oracle, dtype, K):
    pr = tie_problem(dtype)
    for req in (DEFAULT, TOPK8, ("p",)):
        off = calc(oracle, pr, K, dtype, req)
        for seed in SEEDS:
            on = calc(oracle, pr, K, dtype, req, noise=True, seed=seed)
            assert not any(np.isnan(arr).any() for arr in on.values()), (req, seed)
            changed = ~np.all([per_user(same_bits(on[nm], off[nm]), 300) for nm in on], axis=0)
            assert changed.sum() >= 100 and changed[::3].all(), (req, seed, int(changed.sum()))


def test_the_batched_problem_is_built_the_same_way(oracle):
    pr = tie_problem(F32, 2600, 2000, 16)
    assert pr["A"].shape == (2600, 16) and pr["B"].shape == (2000, 16)
    off = calc(oracle, pr, 10, F32, DEFAULT)
    on = calc(oracle, pr, 10, F32, DEFAULT, noise=True, seed=SEEDS[0])
    assert user_is_nan(off)[::3].all() and not any(np.isnan(arr).any() for arr in on.values())
    assert user_is_nan(off)[1500:].sum() > 300         # (both batches of 1,500 and both shards hold such users)


# ---- 4. long test rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_long_rows_are_what_they_should_be(oracle, dtype):
    pr = long_rows_problem(dtype)
    assert pr["A"].shape == (52, 24) and pr["B"].shape == (9037, 24)
    tep, tei, tev = pr["test"]
    trp, tri = pr["train"]
    assert list(np.diff(tep)) == list(LONG_ROWS) * 4
    shared = np.array([np.intersect1d(tri[trp[u]:trp[u + 1]], tei[tep[u]:tep[u + 1]]).size for u in range(52)])
    assert (shared[::3] > 0).all() and shared.sum() == shared[::3].sum()
    kinds = [tev[tep[u]:tep[u + 1]] for u in (9, 22, 35, 48)]                  # the 600-item row of each kind
    assert (kinds[0] <= 0).any() and kinds[1].min() == 1 and (kinds[2] < 0).any() and (kinds[3] == 2).all()
    for K in (10, 65, 100, 256):
        out = calc(oracle, pr, K, dtype, TOPK8)
        assert np.isfinite(out["NDCG@K"]).sum() >= 48 and np.isfinite(out["P@K"]).all()


# ---- the oracle against the compiled reference, under the requests ------------------------------------------------------------------
def _reference_or_skip():
    from oracle.oracle import Reference, reference_available
    if not reference_available():
        pytest.skip("oracle/_ref/librecometrics_ref.so is not built here (the reference's sources are absent): the oracle is not "
                    "compared with the compiled reference under these requests")
    return Reference()


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", EDGE_K)
def test_oracle_equals_the_reference_on_the_edge_users(oracle, dtype, K):
    """every request, noise off and (DEFAULT, TOPK8) on, and the eligibility options: NaN masks identical, and every user whose
    values differ has an exact tie on a positive (i.i.d. factors: next to nobody)"""
    ref = _reference_or_skip()
    differing = 0
    for req in REQUESTS:
        differing += oracle_against_reference(oracle, ref, edge_problem(dtype, K), K, dtype, req)
        if req in (DEFAULT, TOPK8):
            differing += oracle_against_reference(oracle, ref, edge_problem(dtype, K), K, dtype, req, noise=True, seed=7)
        if K == 10:
            for opts in (dict(cold=False), dict(min_pos_test=3), dict(min_items_pool=50), dict(cold=False, min_pos_test=3, min_items_pool=50)):
                differing += oracle_against_reference(oracle, ref, edge_problem(dtype, K, cold_rows=True), K, dtype, req, **opts)
    assert differing <= 2, "more exact ties than i.i.d. factors can have"


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [10, 100, 300])
def test_oracle_and_reference_hold_the_same_users_invalid_under_ties(oracle, dtype, K):
    """the tie problems: the values depend on the reference's undefined order of equal scores, who is NaN does not"""
    ref = _reference_or_skip()
    for req in TIE_REQUESTS:
        oracle_against_reference(oracle, ref, tie_problem(dtype), K, dtype, req)
        if K <= 100:
            oracle_against_reference(oracle, ref, runs_problem(dtype), K, dtype, req)
    for req in (DEFAULT, TOPK8, ("p",)):
        for seed in SEEDS:
            oracle_against_reference(oracle, ref, tie_problem(dtype), K, dtype, req, noise=True, seed=seed)
    if K == 10:
        for req in TIE_REQUESTS:
            oracle_against_reference(oracle, ref, equal_problem(dtype), K, dtype, req)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [10, 65, 100, 256])
def test_oracle_equals_the_reference_on_long_test_rows(oracle, dtype, K):
    ref = _reference_or_skip()
    differing = 0
    for req in (("ndcg",), DEFAULT, TOPK8):
        differing += oracle_against_reference(oracle, ref, long_rows_problem(dtype), K, dtype, req)
        if K == 10:
            differing += oracle_against_reference(oracle, ref, long_rows_problem(dtype), K, dtype, req, noise=True, seed=9)
    assert differing <= 2, "more exact ties than i.i.d. factors can have"
