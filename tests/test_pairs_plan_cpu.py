"""CPU-only: the pairwise plan of tests/_pairs_plan.py covers what it says, its cases are not empty, and the ROC-AUC rule of
tests/_util.py (`roc_tol`) holds between the oracle's two ways to the same number.

Coverage is recomputed from the table of dimensions, not from the generator.  Non-triviality is asserted on the oracle's own outputs,
so that a case cannot pass on the GPU by evaluating nobody or by an option that decides nothing."""
import itertools

import numpy as np
import pytest

import _pairs as pairs
import _pairs_plan as plan
from _parity import NT
from _requests import ALL, COLD_USER, ONLY_NDCG_USER, n_users, per_user, unspecified_in_the_reference
from _util import assert_roc, roc_tol, same_bits

CASES = plan.CASES
IDS = [plan.case_id(c) for c in CASES]


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_the_plan_is_the_same_list_every_time():
    assert plan._generate() == CASES and len(set(CASES)) == len(CASES)
    assert 35 <= len(CASES) <= 50, len(CASES)                 # (35: request x k_metrics)
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        assert all(getattr(c, d) in plan.DIMENSIONS[d] for d in plan.NAMES), c
    for triple in plan.REQUIRED:
        assert any(all(getattr(c, d) == lv for d, lv in triple) for c in CASES), triple


def all_pairs():
    dims = plan.DIMENSIONS
    wanted = {frozenset([(d1, l1), (d2, l2)]) for d1, d2 in itertools.combinations(dims, 2) for l1 in dims[d1] for l2 in dims[d2]}
    assert len(wanted) == sum(len(dims[a]) * len(dims[b]) for a, b in itertools.combinations(dims, 2))
    return wanted


# the two pairs no call can have, and the one the family's 200 users cannot: a batch from factors holds whole 1,024s of users
EXCLUDED = {frozenset([("entry", "scores"), ("noise", "on")]), frozenset([("entry", "scores"), ("splits", "3")]),
            frozenset([("entry", "factors"), ("batches", "64")])}


def test_every_allowed_pair_of_levels_is_in_some_case():
    """every pair but the three excluded ones and the two that those leave no case for; the latter are recomputed here from the
    excluded ones over every combination of levels, so the plan cannot declare a pair unreachable that some case could hold"""
    dims = plan.DIMENSIONS
    assert {frozenset((a, b)) for a, b, why in plan.EXCLUDED if why} == EXCLUDED and len(plan.EXCLUDED) == 3
    under_a_rule = sorted({d for pair in EXCLUDED for d, _ in pair}, key=plan.NAMES.index)
    assert under_a_rule == ["entry", "noise", "batches", "splits"]
    possible = set()                                           # (a pair is possible if some choice of the dimensions under a rule holds it
    for choice in itertools.product(*[dims[d] for d in under_a_rule]):      # and no excluded pair; the other dimensions are free)
        levels = list(zip(under_a_rule, choice))
        held = {frozenset(p) for p in itertools.combinations(levels, 2)}
        if not held & EXCLUDED:
            possible |= held
    ruled = {p for p in all_pairs() if all(d in under_a_rule for d, _ in p)}
    unreachable = ruled - possible - EXCLUDED
    assert unreachable == {frozenset([("noise", "on"), ("batches", "64")]), frozenset([("batches", "64"), ("splits", "3")])}
    assert {frozenset((a, b)) for a, b, _ in plan.UNREACHABLE} == unreachable and len(plan.UNREACHABLE) == 2
    met = set()
    for c in CASES:
        levels = [(d, getattr(c, d)) for d in dims]
        met |= {frozenset(p) for p in itertools.combinations(levels, 2)}
    assert not met & (EXCLUDED | unreachable), "a case holds an excluded pair"
    missing = all_pairs() - EXCLUDED - unreachable - met
    assert not missing, "pairs no case holds: %s" % sorted(sorted(p) for p in missing)[:8]


def test_the_batches_of_the_score_entry_are_several():
    """batches = 64 cuts the 200 users into 64 / 64 / 64 / 8 and a shard's 66 or 67 into 64 + 2 or 3: more than one batch either way"""
    assert plan.batch_cuts(200, 64) == [0, 64, 128, 192, 200] and plan.batch_cuts(66, 64) == [0, 64, 66] and plan.batch_cuts(67, 64) == [0, 64, 67]
    assert plan.batch_cuts(200, None) == [0, 200] and plan.batch_cuts(64, 64) == [0, 64] and plan.batch_cuts(128, 64) == [0, 64, 128]
    assert plan.shard_ranges(200, 1) == [(0, 200)] and plan.shard_ranges(200, 3) == [(0, 66), (66, 133), (133, 200)]
    for c in CASES:
        if c.batches == "64":
            assert c.entry == "scores" and all(len(cuts) > 2 for cuts in plan.cuts_of(c, pairs.M_USERS)), c
        else:
            assert all(len(cuts) == 2 for cuts in plan.cuts_of(c, pairs.M_USERS)), c


def test_the_cases_left_out_as_empty_are_empty(oracle):
    """plan.EMPTY: k_metrics = 1, no ROC-AUC, no noise -- nobody is valid, whatever the scores"""
    assert len(plan.EMPTY) == 5
    for triple in plan.EMPTY:
        req = plan.REQUESTS[dict(triple)["request"]]
        assert dict(triple)["K"] == 1 and dict(triple)["noise"] == "off" and "roc" not in req
        for structure in plan.DIMENSIONS["structure"]:
            pr = pairs.problem(np.float32, 1, structure, "none")
            out = pairs.want(oracle, pr, 1, np.float32, metrics=req)
            assert all(np.isnan(arr).all() for arr in out.values()), (req, structure)
    for c in CASES:
        assert plan.is_valid(dict(zip(plan.NAMES, c))), c


# ---- the problems -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", plan.DIMENSIONS["K"])
def test_the_rows_are_what_the_plan_says(dtype, K):
    n = pairs.N_ITEMS
    pr = pairs.problem(dtype, K, "iid", "none")
    assert pr["A"].shape == (200, 20) and pr["B"].shape == (n, 20) and pr["A"].dtype == dtype
    trp, tri = pr["train"]
    tep, tei, tev = pr["test"]
    ntr, nte = np.diff(trp), np.diff(tep)
    assert list(nte[:6]) == [0, 1, 63, 64, 618, 618] and ntr[6] == n
    assert list(n - ntr[7:11]) == [1, max(1, K - 1), K, K + 1]
    assert ntr[ONLY_NDCG_USER] + nte[ONLY_NDCG_USER] == n and ntr[COLD_USER] == 0 and nte[COLD_USER] == 7
    shared = lambda p, u: np.intersect1d(p["train"][1][p["train"][0][u]:p["train"][0][u + 1]], p["test"][1][p["test"][0][u]:p["test"][0][u + 1]]).size
    assert shared(pr, 11) == 4 and shared(pr, ONLY_NDCG_USER) == 0
    assert (tev[tep[13]:tep[14]] == 0).all() and (tev[tep[12]:tep[13]] < 0).any()
    assert set(range(1, 20)) <= set(nte.tolist()), "short test rows of many lengths"
    over = pairs.problem(dtype, K, "iid", "third")
    assert (np.diff(over["test"][0]) == nte).all() and (over["test"][1] == tei).all()
    for u in range(200):
        if u in pairs.OVERLAP_USERS:                           # (user 11 shares four items already)
            assert -(-3 * int(nte[u]) // 10) <= shared(over, u) <= -(-3 * int(nte[u]) // 10) + shared(pr, u), u
        else:
            assert shared(over, u) == shared(pr, u), u
    assert np.diff(over["train"][0])[COLD_USER] == 0
    for p in (pr, over):                                       # sorted rows without duplicates
        for ptr, idx in (p["train"], p["test"][:2]):
            d = np.diff(idx.astype(np.int64))
            inner = np.ones(idx.shape[0] - 1, bool)
            inner[ptr[1:-1][(ptr[1:-1] > 0) & (ptr[1:-1] < idx.shape[0])] - 1] = False
            assert (d[inner] > 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_score_structures_are_what_the_plan_says(oracle, dtype):
    S = {st: pairs.scores(oracle, pairs.problem(dtype, 10, st, "none"), dtype) for st in plan.DIMENSIONS["structure"]}
    assert all(s.shape == (200, pairs.N_ITEMS) and np.isfinite(s).all() for s in S.values())
    assert (np.diff(S["ascending"], axis=1) > 0).all()
    d = np.diff(S["runs"], axis=1)
    flipped = np.zeros(200, bool)
    flipped[pairs.RUNS_FLIPPED] = True
    assert (d[~flipped] >= 0).all() and (d[flipped] <= 0).all() and 0.7 < (d == 0).mean() < 0.9, "exact ties in runs"
    head = S["runs"][:, :pairs.RUNS_HEAD]
    assert (head == head[:, :1]).all() and (S["runs"][flipped].max(axis=1) == head[flipped, 0]).all(), "the flipped users' best run"
    assert ((S["runs"][~flipped] == S["runs"][~flipped].max(axis=1, keepdims=True)).sum(axis=1) < 10).all()
    zone = np.abs(S["runs"]) < 2.0 ** -14
    assert 0.01 < zone.mean() < 0.2 and zone.any(axis=1).all(), "part of every user's ramp lies where the fp32 noise reorders"
    zero = (S["zero_rows"] == 0).all(axis=0)
    assert 0.1 < zero.mean() < 0.2 and (S["zero_rows"][:, ~zero] != 0).mean() > 0.999
    assert 100 < zero.sum() < 300 and (S["zero_rows"][pairs.ZERO_TOP].max(axis=1) == 0).all(), "every third user: the zeros are the best scores"
    assert len(pairs.ZERO_TOP) == 66 and S["zero_rows"][COLD_USER].max() > 0
    assert (np.sort(S["iid"], axis=1)[:, 1:] != np.sort(S["iid"], axis=1)[:, :-1]).mean() > 0.999


# ---- non-triviality, on the oracle's outputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_case_is_not_trivial(oracle, case):
    pr, K, dtype, kw = pairs.problem_of(case), case.K, pairs.DTYPE[case.dtype], plan.call_kw(case)
    m = n_users(pr)
    req = plan.REQUESTS[case.request]
    out = pairs.want_of(oracle, case)
    assert len(out) == len(req)
    first = next(iter(out.values()))                           # (the oracle returns the outputs in the request's order)
    alive = ~per_user(np.isnan(first), m)
    assert alive.sum() >= m // 2, "only %d of %d users have a first requested output" % (alive.sum(), m)
    ev = pairs.evaluated(pr, K, **kw)
    assert not (alive & ~ev).any(), "the eligibility rules as restated here hold users %s out" % np.flatnonzero(alive & ~ev)[:8].tolist()

    if case.eligibility == "strict":
        lax = pairs.want_of(oracle, case, cold=True, min_pos_test=1, min_items_pool=2)
        lost = [u for u in range(m) if all(np.isnan(out[nm][u]).all() for nm in out) and not all(np.isnan(lax[nm][u]).all() for nm in out)]
        assert lost, "the eligibility keywords hold nobody out"
        if not (case.noise == "off" and "roc" not in req and case.structure == "runs"):
            assert COLD_USER in lost                           # (cold=False; on `runs` the partial rule may have held it invalid already)

    if case.overlap == "third":
        trp, tri = pr["train"]
        tep, tei = pr["test"][:2]
        hit = [u for u in np.flatnonzero(alive) if np.intersect1d(tri[trp[u]:trp[u + 1]], tei[tep[u]:tep[u + 1]]).size]
        assert len(hit) >= 10, "evaluated users with a test item in their train row: %s" % hit

    if case.noise == "on" and case.structure in ("runs", "zero_rows"):
        off = pairs.want_of(oracle, case, noise=False, seed=1)
        changed = ~np.all([per_user(same_bits(out[nm], off[nm]), m) for nm in out], axis=0)
        assert changed.any(), "the noise changes nobody's outputs"

    if unspecified_in_the_reference(req):
        users_told_from_the_all_ten_call(oracle, case)


def users_told_from_the_all_ten_call(oracle, case):
    """A request under deviation D1 / D2 against the all-ten call, in the outputs both define.  Without ROC-AUC the ranking is only
    partially sorted and a user is invalid when its best and its K-th score are equal (the partial rule); with the noise on no such
    rule applies.  So: where an evaluated user's best K candidates are exactly tied and the noise is off, the request must tell that
    user from the all-ten call; everywhere else it must change nobody.  Returns the number of users told apart."""
    pr, K, dtype, kw = pairs.problem_of(case), case.K, pairs.DTYPE[case.dtype], plan.call_kw(case)
    m = n_users(pr)
    out, full = pairs.want_of(oracle, case), pairs.want_of(oracle, case, metrics=ALL)
    differs = ~np.all([per_user(same_bits(out[nm], full[nm]), m) for nm in out], axis=0)
    S = pairs.scores(oracle, pr, dtype).copy()
    trp, tri = pr["train"]
    S[np.repeat(np.arange(m), np.diff(trp)), tri] = -np.inf
    top = -np.sort(-S, axis=1)[:, :K]
    tied = pairs.evaluated(pr, K, **kw) & (pr["B"].shape[0] - np.diff(trp) > K) & (top[:, 0] == top[:, -1]) & (case.noise == "off")
    full_alive = ~np.all([per_user(np.isnan(full[nm]), m) for nm in out], axis=0)
    assert (differs == (tied & full_alive)).all(), (np.flatnonzero(differs)[:8].tolist(), np.flatnonzero(tied & full_alive)[:8].tolist())
    return int(differs.sum())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("request_name", ["pr", "hit+rr"])
def test_requests_under_d1_d2_differ_from_the_all_ten_call_on_the_runs(oracle, dtype, request_name):
    """the plan's own problem on which the partial validity rule decides: `runs`, noise off -- the flipped users' best scores are one
    run, invalid under ("pr",) and ("hit", "rr") and valid under the all-ten call; and the plan holds such a case for either request"""
    pr = pairs.problem(dtype, 10, "runs", "none")
    req = plan.REQUESTS[request_name]
    out, full = pairs.want(oracle, pr, 10, dtype, metrics=req), pairs.want(oracle, pr, 10, dtype, metrics=ALL)
    differs = ~np.all([per_user(same_bits(out[nm], full[nm]), 200) for nm in out], axis=0)
    assert 50 <= differs.sum() < 100, int(differs.sum())
    in_plan = [users_told_from_the_all_ten_call(oracle, c) for c in CASES if c.request == request_name]
    assert max(in_plan) >= 50, in_plan


# ---- the premise of roc_tol ---------------------------------------------------------------------------------------------------------
def roc_from_ranks(rank, pr, dtype):
    """T(1 - float64(S - P (P + 1) / 2) / float64(P N)) from oracle.rank's exact positive ranks, in the reference's unsigned
    64-bit integers (a test item inside the train row has no rank and still counts as a positive: the difference wraps)"""
    trp, tep = pr["train"][0], pr["test"][0]
    m = tep.shape[0] - 1
    out = np.full(m, np.nan, dtype)
    mask = (1 << 64) - 1
    for u in range(m):
        if rank["status"][u]:
            continue
        P = int(tep[u + 1] - tep[u])
        C = pr["B"].shape[0] - int(trp[u + 1] - trp[u])
        S = int(rank["pos_rank"][tep[u]:tep[u + 1]].sum())
        x, y = (S - P * (P + 1) // 2) & mask, (P * ((C - P) & mask)) & mask
        with np.errstate(divide="ignore", invalid="ignore"):
            out[u] = dtype(np.float64(1.0) - np.float64(x) / np.float64(y))
    return out


ROC_CASES = [c for c in CASES if "roc" in plan.REQUESTS[c.request]]


@pytest.mark.parametrize("case", ROC_CASES, ids=[plan.case_id(c) for c in ROC_CASES])
def test_roc_auc_from_the_exact_ranks_is_within_the_rule_of_the_oracle(oracle, case):
    """the oracle forms ROC-AUC in long double, as the reference does; the device forms it in fp64 from the same integers.  The fp64
    formula on oracle.rank's ranks -- what a device with every rank right returns -- lies within roc_tol of oracle.calc, noise off and on"""
    pr, K, dtype = pairs.problem_of(case), case.K, pairs.DTYPE[case.dtype]
    kw = {k: v for k, v in plan.call_kw(case).items() if k in ("cold", "min_items_pool", "min_pos_test")}
    users = 0
    for noise in (False, True):
        nk = dict(kw, noise=noise, seed=plan.NOISE_SEED)
        rank = oracle.rank(pr["A"], pr["B"], pr["train"], pr["test"], K, dtype=dtype, nthreads=NT, **nk)
        want = pairs.want(oracle, pr, K, dtype, metrics=("roc",), **nk)["ROC_AUC"]
        mine = roc_from_ranks(rank, pr, dtype)
        assert_roc(mine, want, dtype, "%s noise=%s" % (pr.name, noise))
        users += int(np.isfinite(want).sum())
    assert users >= 200
    assert roc_tol(np.float32) == np.finfo(np.float32).eps and roc_tol(np.float64) == np.finfo(np.float64).eps


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_miscounted_rank_is_beyond_the_rule(oracle, dtype):
    """what the rule sees: one positive of a user one rank too low moves ROC-AUC by 1 / (P x negatives) -- beyond roc_tol for every
    evaluated user of this family (P x negatives < 2^23, so also in fp32), and below the former 1e-5 for the streamed users"""
    pr, K = pairs.problem(dtype, 10, "iid", "none"), 10
    rank = oracle.rank(pr["A"], pr["B"], pr["train"], pr["test"], K, dtype=dtype, nthreads=NT)
    want = pairs.want(oracle, pr, K, dtype, metrics=("roc",))["ROC_AUC"]
    tep = pr["test"][0]
    bumped = dict(rank, pos_rank=rank["pos_rank"].copy())
    ranked = np.flatnonzero((rank["status"] == 0) & np.isfinite(want))
    for u in ranked:
        row = bumped["pos_rank"][tep[u]:tep[u + 1]]
        row[np.flatnonzero(row)[0]] += 1
    off = roc_from_ranks(bumped, pr, dtype)
    d = np.abs(off.astype(np.float64) - want.astype(np.float64))[ranked] / np.maximum(1.0, np.abs(want[ranked].astype(np.float64)))
    assert ranked.shape[0] >= 150 and (d > roc_tol(dtype)).all(), "a miscount the rule does not see: users %s" % ranked[d <= roc_tol(dtype)][:8].tolist()
    streamed = np.isin(ranked, [4, 5])                         # 618 test items among 1,237
    assert streamed.sum() == 2 and (d[streamed] < 1e-5).all() and (d[~streamed] > d[streamed].max()).all()
