"""What the tests of metric REQUESTS share (tests/test_requests_cpu.py, tests/test_hip_requests.py): the requests, the problems and
the checker of one (problem, K, dtype, request) case.

A request is the set of metrics a call asks for.  Without ROC-AUC three rules of the reference change (oracle/recometrics_oracle.cpp
`eval_user`, reference src/recometrics.hpp:439-563):

* eligibility by request -- a user whose train and test rows cover the catalogue is evaluated only when NDCG is asked for; a user
  with candidates <= K only when one of ROC / PR / AP / TAP / RR is;
* the partial validity rule -- with K < candidates the ranking is only partially sorted, and a user is invalid when its best and
  its K-th score are equal, not when all of its scores are;
* tie noise -- without the AUCs no positives' kernel flags a user for the exact pass: only the finalisation's scan of the list does.

The problems below make each rule decide somebody's outputs; tests/test_requests_cpu.py asserts on the oracle's outputs that they do.
"""
import functools
import os

import numpy as np

from _parity import NT, TOL, _check_against_oracle, _reference, hip_calc
from _util import assert_close, assert_roc, assert_same_bits, same_bits
from oracle.ties import tie_pairs_per_user

F32, F64 = np.float32, np.float64
ALL = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr")
DEFAULT = ("p", "ap", "ndcg")                            # calc_reco_metrics with every keyword at its default
TOPK8 = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr")
REQUESTS = (DEFAULT, TOPK8, ("p",), ("ndcg",), ("p", "ndcg"), ("hit", "rr"), ("tp", "r"), ("ap", "tap"), ("pr",), ("p", "pr"), ("p", "roc"))
TIE_REQUESTS = (DEFAULT, ("pr",), ("p", "pr"), ("p", "roc"), TOPK8)


def req_id(req):
    return {DEFAULT: "default", TOPK8: "topk8", ALL: "all"}.get(tuple(req), "+".join(req))


def unspecified_in_the_reference(req):
    """outputs of a request whose VALUES the reference leaves undefined (DESIGN.md deviations D1, D2): Hit@K / RR@K asked for without
    any of P / TP / R / AP / TAP / NDCG stay uninitialised there; PR-AUC without ROC-AUC is walked over a partially sorted list.
    Who is NaN is defined all the same."""
    out = set()
    if not set(req) & {"p", "tp", "r", "ap", "tap", "ndcg"}:
        out |= {"Hit@K", "RR@K"}
    if "pr" in req and "roc" not in req:
        out.add("PR_AUC")
    return out


# ---- problems ---------------------------------------------------------------------------------------------------------------------
class Problem(dict):
    """the dict of synth.make_problem (A, B, train, test) with a name; hashable by identity (the builders below are cached), so that
    the all-ten results can be cached per problem.  `ties`: exact ties are planted -- the reference's order of them is undefined (D4)"""
    def __init__(self, name, pr, ties=False):
        super().__init__(pr)
        self.name, self.ties = name, ties

    __hash__ = object.__hash__
    __eq__ = object.__eq__


def csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return indptr, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)


def replace_rows(pr, n, rows, dtype):
    """the problem with the users of `rows` = {user: (train items, test items, test values or None)} replaced"""
    trp, tri = pr["train"]
    tep, tei, tev = pr["test"]
    m = trp.shape[0] - 1
    TR, TE, TV = [], [], []
    for u in range(m):
        if u in rows:
            a, b, v = rows[u]
            a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
            v = np.arange(1, b.shape[0] + 1, dtype=dtype) if v is None else np.asarray(v, dtype)
        else:
            a, b, v = tri[trp[u]:trp[u + 1]], tei[tep[u]:tep[u + 1]], tev[tep[u]:tep[u + 1]]
        TR.append(a); TE.append(b); TV.append(v)
    p = np.zeros(m + 1, np.int64); q = np.zeros(m + 1, np.int64)
    np.cumsum([x.shape[0] for x in TR], out=p[1:]); np.cumsum([x.shape[0] for x in TE], out=q[1:])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return dict(A=pr["A"], B=pr["B"], train=(p.astype(np.int32), cat(TR, np.int32)), test=(q.astype(np.int32), cat(TE, np.int32), cat(TV, dtype)))


@functools.lru_cache(maxsize=64)
def planted_problem(m, n, kf, dtype, seed, K):
    """i.i.d. factors and make_interactions rows; from 33 users on, the edge users planted in one problem: no test item; 1, 63, 64,
    1,023 and 1,500 test items (as many as half of the catalogue allows); a train row that is the whole catalogue; one candidate;
    C = K - 1, K, K + 1 candidates; test items that are train items; negative and zero test values"""
    from recometrics_amd.synth import make_problem
    pr = make_problem(m, n, kf, dtype, mean_c=max(2, min(40, n // 8)), seed=seed)
    if m < 33 or n < 16:
        return pr
    rng = np.random.default_rng(seed + 1)
    items = np.arange(n, dtype=np.int32)
    rows = {}

    def split(n_test, n_train=None):
        pick = rng.permutation(n)
        n_test = max(1, min(n_test, n // 2))
        n_train = min(40, n // 8) if n_train is None else n_train
        return np.sort(pick[n_test:n_test + n_train]), np.sort(pick[:n_test]), None
    rows[0] = (split(1)[0], np.zeros(0, np.int32), None)
    for u, cnt in zip((1, 2, 3, 4, 5), (1, 63, 64, 1023, 1500)):
        rows[u] = split(cnt)
    rows[6] = (items, np.sort(rng.permutation(n)[:3]), None)                     # the train row is the whole catalogue
    for u, C in zip((7, 8, 9, 10), (1, K - 1, K, K + 1)):
        C = max(1, min(C, n))
        cand = np.sort(rng.permutation(n)[:C])
        rows[u] = (np.setdiff1d(items, cand).astype(np.int32), cand[:max(1, C // 2)], None)
    tr, te, _ = split(9)
    rows[11] = (np.sort(np.concatenate([tr, te[:4]])), te, None)                 # four test items are train items too
    tr, te, _ = split(6)
    rows[12] = (tr, te, np.array([-3.0, 0.0, 2.0, 0.0, -1.0, 5.0][:te.shape[0]]))
    tr, te, _ = split(5)
    rows[13] = (tr, te, np.zeros(te.shape[0]))
    return replace_rows(pr, n, rows, dtype)


ONLY_NDCG_USER, COLD_USER = 14, 15


@functools.lru_cache(maxsize=None)
def edge_problem(dtype, K, cold_rows=False):
    """129 users x 1,000 items x 16 factors: planted_problem's edge users 0-13 (planted for this K), user 14 whose train and test rows
    are disjoint and cover the catalogue between them (40 test items: evaluated for NDCG alone), user 15 without a train row.
    `cold_rows`: users 20-22 lose their train rows too (the problem of test_hip_scores.test_eligibility_options)"""
    n = 1000
    pr = planted_problem(129, n, 16, dtype, 11, K)
    rng = np.random.default_rng(1400)
    te = np.sort(rng.permutation(n)[:40])
    tep, tei = pr["test"][:2]
    rows = {ONLY_NDCG_USER: (np.setdiff1d(np.arange(n), te), te, None),
            COLD_USER: (np.zeros(0, np.int32), np.sort(rng.permutation(n)[:7]), None)}
    if cold_rows:
        rows.update({u: (np.zeros(0, np.int32), tei[tep[u]:tep[u + 1]], None) for u in (20, 21, 22)})
    return Problem("edge users K=%d%s" % (K, " +cold rows" if cold_rows else ""), replace_rows(pr, n, rows, dtype))


@functools.lru_cache(maxsize=None)
def tie_problem(dtype, m=300, n=5000, kf=20):
    """make_problem's rows with non-negative item factors, 15 % of the items all-zero, and every third user's factors non-positive:
    for those users every score is <= 0 and the cold items' exact zeros -- about 750 of them -- are tied at the top of the ranking,
    far beyond any K; their other scores differ, so the full rule (best == worst) holds them valid and the partial rule does not"""
    from recometrics_amd.synth import make_problem
    pr = make_problem(m, n, kf, dtype, mean_c=80, seed=41)
    B = np.abs(pr["B"])
    B[np.random.default_rng(5).random(n) < 0.15] = 0
    A = pr["A"].copy()
    A[::3] = -np.abs(A[::3])
    return Problem("ties %dx%d" % (m, n), dict(pr, A=A, B=B), ties=True)


@functools.lru_cache(maxsize=None)
def runs_problem(dtype):
    """synth's `runs` with 39 of 40 item rows equal to their predecessor's: the ascending ramp in runs of about 40 exactly equal
    scores (the same runs for every user, cut differently by each train row) -- K = 10 ends inside the best run for most users,
    K = 100 beyond it"""
    from recometrics_amd.synth import make_structured
    return Problem("runs", make_structured("runs", 150, 4000, 40, dtype, mean_c=60, seed=23, dup=0.975), ties=True)


@functools.lru_cache(maxsize=None)
def equal_problem(dtype):
    """every item the same factors: every candidate of a user the same score"""
    from recometrics_amd.synth import make_problem
    pr = make_problem(129, 1000, 16, dtype, mean_c=30, seed=43)
    B = np.repeat(pr["B"][:1], 1000, axis=0)
    return Problem("all equal", dict(pr, B=np.ascontiguousarray(B)), ties=True)


LONG_ROWS = (1, 40, 63, 64, 65, 100, 255, 256, 257, 600, 2047, 2048, 4000)


@functools.lru_cache(maxsize=None)
def long_rows_problem(dtype):
    """52 users x 9,037 items x 24 factors, test rows of 1 ... 4,000 items around 64, 256 and 2,048; test values with zeros and
    negatives, without, and all tied (the three kinds of test_ideal_dcg_with_k_metrics_beyond_the_finalize_buffer); every third
    user has test items -- the first, the middle and the last of its row -- in its train row as well"""
    from recometrics_amd.synth import make_factors
    rng = np.random.default_rng(404)
    m, n, k = 52, 9037, 24
    A, B = make_factors(m, n, k, dtype, seed=44)
    rows_tr, rows_te, vals = [], [], []
    for u in range(m):
        nte = LONG_ROWS[u % len(LONG_ROWS)]
        items = rng.permutation(n)[: nte + 150]
        te, tr = np.sort(items[:nte]), np.sort(items[nte:])
        if u % 3 == 0:
            tr = np.union1d(tr, te[[0, nte // 2, nte - 1]])
        kind = u // len(LONG_ROWS)
        v = rng.integers(-3, 6, size=nte) if kind % 2 == 0 else rng.integers(1, 4, size=nte)
        if kind == 3 and nte > 2:
            v[:] = 2
        rows_te.append(te); rows_tr.append(tr); vals.append(v.astype(dtype))
    tep, tei = csr(rows_te)
    return Problem("long rows", {"A": A, "B": B, "train": csr(rows_tr), "test": (tep, tei, np.concatenate(vals).astype(dtype))})


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def n_users(pr):
    return pr["test"][0].shape[0] - 1


def per_user(x, m):
    return x.reshape(m, -1).all(axis=1)


def user_is_nan(out, names=None):
    """per user: every requested output (of `names`) is NaN in every column"""
    names = list(out) if names is None else [nm for nm in names if nm in out]
    m = out[names[0]].shape[0]
    return np.all([per_user(np.isnan(out[nm]), m) for nm in names], axis=0)


@functools.lru_cache(maxsize=None)
def oracle_all(oracle, pr, K, dtype, cumulative, kw):
    return oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, cumulative=cumulative, dtype=dtype, nthreads=NT, **dict(kw))


@functools.lru_cache(maxsize=None)
def _hip_all(hip, pr, K, dtype, cumulative, kw, env):
    return hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, cumulative=cumulative, dtype=dtype, **dict(kw))


def hip_all(hip, pr, K, dtype, cumulative, kw):
    """the all-ten call, once per problem and set of library switches"""
    env = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("RM_")))
    return _hip_all(hip, pr, K, dtype, cumulative, kw, env)


def compare_with_reference(mine, real, pr, scores_of, dtype, noise, what, skip=(), exact_order=True):
    """_parity's rule for one pair of outputs: NaN masks equal for every output; beyond `skip` every value within TOL, and every
    user that differs in a bit (ROC-AUC: by more than TOL -- x87 long double there) has a candidate whose score equals one of its
    positives' exactly (oracle/ties.py), each such pair worth one rank of ROC-AUC.  `exact_order=False`: the masks alone (planted
    ties: the reference's order of them is undefined)."""
    m = n_users(pr)
    assert set(mine) == set(real), what
    differing = np.zeros(m, bool)
    d_roc = np.zeros(m)
    for name in real:
        if name in skip and name != "PR_AUC" and mine[name].ndim == 2:
            # (D1, cumulative: the reference never walks the list for Hit@K / RR@K alone, and its override for candidates <= K then
            # fills a row with NaN that the restatement's walk has written -- quirk Q4 on a walk that did not happen)
            continue
        bad = np.isnan(mine[name]) != np.isnan(real[name])
        assert not bad.any(), "%s: %s: NaN mask differs from the compiled reference's at %s" % (what, name, np.argwhere(bad)[:5].tolist())
        if name in skip or not exact_order:
            continue
        if name == "ROC_AUC":
            r64 = np.nan_to_num(real[name].astype(np.float64))
            d_roc = np.abs(np.nan_to_num(mine[name].astype(np.float64)) - r64) / np.maximum(1.0, np.abs(r64))
            differing |= d_roc > TOL
        else:
            differing |= ~per_user(same_bits(mine[name], real[name]), m)
    pairs = np.zeros(m, np.int64)
    if differing.any():
        who = np.flatnonzero(differing)
        pairs[who] = tie_pairs_per_user(scores_of(who), pr["train"], pr["test"], who, noise_zone=(2.0 ** -14 if noise and dtype == F32 else None))
        assert (pairs[who] > 0).all(), "%s: users %s differ from the compiled reference without an exact tie on a positive" % (what, who[pairs[who] == 0][:8].tolist())
    npos = np.diff(pr["test"][0]).astype(np.float64)
    nneg = np.maximum(pr["B"].shape[0] - np.diff(pr["train"][0]) - npos, 1)
    assert (d_roc <= TOL + pairs / np.maximum(npos * nneg, 1)).all(), "%s: ROC_AUC vs the compiled reference: %g" % (what, d_roc.max())
    return int(differing.sum())


def check_request(hip, oracle, pr, K, dtype, req, **kw):
    """One problem, one K, one dtype, one request; kw: noise, seed, cold, min_items_pool, min_pos_test.  Single and cumulative.
    Returns the device's single outputs."""
    req = tuple(req)
    m = n_users(pr)
    noise = bool(kw.get("noise"))
    kw_key = tuple(sorted(kw.items()))
    ref = _reference()
    skip = unspecified_in_the_reference(req)
    single = None
    for cum in (False, True):
        what = "%s K=%d %s %s cumulative=%s %s" % (pr.name, K, np.dtype(dtype).name, req_id(req), cum, kw)
        # 1. the oracle, bitwise (ROC-AUC, formed in x87 long double by the reference and in fp64 here: an ulp, _util.roc_tol)
        want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, cumulative=cum, dtype=dtype, nthreads=NT, **kw)
        got = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, cumulative=cum, dtype=dtype, **kw)
        assert set(got) == set(want) and len(got) == len(req), what
        for name in want:
            if name == "ROC_AUC":
                assert_roc(got[name], want[name], dtype, what + ": " + name)
            else:
                assert_same_bits(got[name], want[name], what + ": " + name)
        # 2. the compiled reference on what it defines: who is NaN -- always; the values -- where no exact ties are planted (the
        #    whole comparison of _parity for a request it defines entirely, the same rule without the outputs of D1 / D2 otherwise)
        if ref is not None:
            real = ref.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, cumulative=cum, dtype=dtype, nthreads=NT, **kw)
            if skip or pr.ties:
                scores_of = lambda who: hip.debug_scores(np.ascontiguousarray(pr["A"][who], dtype), np.ascontiguousarray(pr["B"], dtype))
                compare_with_reference(got, real, pr, scores_of, dtype, noise, what, skip=skip, exact_order=not pr.ties)
            if pr.ties and noise and dtype == F64:          # the noise separates every pair of fp64 scores: the order is defined
                for name in real:
                    if name not in skip:
                        assert_close(got[name], real[name], TOL, what + ": " + name + " vs the compiled reference, noise on")
                        if name != "ROC_AUC":
                            assert_same_bits(got[name], real[name], what + ": " + name + " vs the compiled reference, noise on (bitwise)")
        # 3. against the all-ten call: the device changes a user's value between the requests exactly where the oracle does
        got_all = hip_all(hip, pr, K, dtype, cum, kw_key)
        want_all = oracle_all(oracle, pr, K, dtype, cum, kw_key)
        for name in want:
            if name == "ROC_AUC":
                continue
            dev = per_user(same_bits(got[name], got_all[name]), m)
            orc = per_user(same_bits(want[name], want_all[name]), m)
            assert (dev == orc).all(), "%s: %s: the request changes users %s on the device and users %s in the oracle" % (
                what, name, np.flatnonzero(~dev)[:8].tolist(), np.flatnonzero(~orc)[:8].tolist())
        if not cum:
            single = got
    if ref is not None:
        # the project's whole comparison: lists and ranks against the oracle, and -- for a request the reference defines entirely,
        # on inputs on which its order is defined -- every value against the reference
        _check_against_oracle(hip, oracle, pr, K, dtype=dtype, reference=not (pr.ties or skip), metrics=req, **kw)
    return single


def oracle_against_reference(oracle, ref, pr, K, dtype, req, **kw):
    """the restatement against the compiled reference under one request (no device): the rule of compare_with_reference"""
    scores = None
    n_diff = 0
    for cum in (False, True):
        what = "%s K=%d %s %s cumulative=%s %s" % (pr.name, K, np.dtype(dtype).name, req_id(req), cum, kw)
        mine = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, cumulative=cum, dtype=dtype, nthreads=NT, **kw)
        real = ref.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, cumulative=cum, dtype=dtype, nthreads=NT, **kw)

        def scores_of(who):
            nonlocal scores
            if scores is None:
                scores = oracle.scores(pr["A"], pr["B"], dtype=dtype)
            return scores[who]
        n_diff += compare_with_reference(mine, real, pr, scores_of, dtype, bool(kw.get("noise")), what,
                                         skip=unspecified_in_the_reference(req), exact_order=not pr.ties)
    return n_diff
