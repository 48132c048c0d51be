"""What the two walks of the pairwise plan share (tests/test_pairs_plan_cpu.py, tests/test_hip_pairs.py): the problem a case runs
on and the oracle's answer to it, each made once.

One family, the scale of tests/test_hip_sweep_rows.py: 200 users x 1,237 items x 20 factors -- two user blocks in fp32 and four in
fp64 with a partial last one, whole 64- and 96-item tiles and a ragged last one.  The rows are _requests.planted_problem's (test rows
of 1 ... 63 items, streamed rows of 64 and 618 items, no test item, a train row that is the whole catalogue, 1 / K - 1 / K / K + 1
candidates, test items that are train items, negative and zero test values) with edge_problem's only-NDCG user and cold user on top."""
import functools

import numpy as np

import _pairs_plan as plan
from _parity import NT
from _requests import COLD_USER, ONLY_NDCG_USER, Problem, planted_problem, replace_rows

M_USERS, N_ITEMS, FACTORS = 200, 1237, 20
SEED = 31
DTYPE = {"f32": np.float32, "f64": np.float64}
OVERLAP_USERS = range(2, M_USERS, 3)             # (2, 5, 8, ...: the cold user, 15, keeps its empty train row)
RUNS_DUP, RUNS_SPAN = 0.8, 2.0 ** -10            # runs of about five equal scores; a sixteenth of the ramp inside the fp32 noise zone
ZERO_TOP = [u for u in range(0, M_USERS, 3) if u != COLD_USER]   # zero_rows: the users whose best scores are the zeros
RUNS_FLIPPED, RUNS_HEAD = slice(1, None, 3), 320 # users 1, 4, 7, ... rank the ramp from its other end, which begins with a run of 320


@functools.lru_cache(maxsize=None)
def rows(dtype, K, overlap):
    """train and test rows: planted for this K, users 14 and 15 as in edge_problem, the overlap on top"""
    n = N_ITEMS
    pr = planted_problem(M_USERS, n, FACTORS, dtype, SEED, K)
    rng = np.random.default_rng(1400)
    te = np.sort(rng.permutation(n)[:40])
    new = {ONLY_NDCG_USER: (np.setdiff1d(np.arange(n), te), te, None),
           COLD_USER: (np.zeros(0, np.int32), np.sort(rng.permutation(n)[:7]), None)}
    pr = replace_rows(pr, n, new, dtype)
    if overlap == "third":
        trp, tri = pr["train"]
        tep, tei, tev = pr["test"]
        new = {}
        for u in OVERLAP_USERS:
            t = tei[tep[u]:tep[u + 1]]
            if t.shape[0]:
                cnt = -(-3 * t.shape[0] // 10)                                   # 30 %, rounded up: evenly spaced through the row
                new[u] = (np.union1d(tri[trp[u]:trp[u + 1]], t[np.arange(cnt) * t.shape[0] // cnt]), t, tev[tep[u]:tep[u + 1]])
        pr = replace_rows(pr, n, new, dtype)
    return pr


@functools.lru_cache(maxsize=None)
def factors(dtype, K, structure):
    from recometrics_amd.synth import make_structured
    if structure in ("iid", "zero_rows"):
        pr = planted_problem(M_USERS, N_ITEMS, FACTORS, dtype, SEED, K)
        A, B = pr["A"], pr["B"]
        if structure == "zero_rows":
            # _requests.tie_problem's way: 15 % of the item rows zero -- ties at 0, inside the fp32 noise zone -- under non-negative
            # item factors, and every third user's factors non-positive: for those users the zeros are tied at the top of the ranking
            B = np.abs(B)
            B[np.random.default_rng(5).random(N_ITEMS) < 0.15] = 0
            # (but the cold user, whom cold=False is to hold out under every request: tied at the top it is invalid without ROC-AUC anyway)
            A = A.copy()
            A[ZERO_TOP] = -np.abs(A[ZERO_TOP])
        return A, B
    if structure == "runs":                                                      # exact ties along the item axis, in fp32 partly below the noise
        pr = make_structured("runs", M_USERS, N_ITEMS, FACTORS, dtype, mean_c=8, seed=SEED, dup=RUNS_DUP, span=RUNS_SPAN)
        # every user's scores follow the one ramp, so everybody's best run is the same run.  Every third user gets the ramp upside
        # down, and the ramp's first RUNS_HEAD items are made one run: those users' best K
        # scores are tied at every k_metrics of the plan, the others' at none but 1
        A, B = pr["A"].copy(), pr["B"].copy()
        A[RUNS_FLIPPED, 0] *= -1
        B[:RUNS_HEAD] = B[0]
        return A, B
    pr = make_structured(structure, M_USERS, N_ITEMS, FACTORS, dtype, mean_c=8, seed=SEED)
    return pr["A"], pr["B"]


@functools.lru_cache(maxsize=None)
def problem(dtype, K, structure, overlap):
    r = rows(dtype, K, overlap)
    A, B = factors(dtype, K, structure)
    name = "pairs %s K=%d %s overlap=%s" % (np.dtype(dtype).name, K, structure, overlap)
    return Problem(name, dict(A=A, B=B, train=r["train"], test=r["test"]), ties=structure in ("runs", "zero_rows"))


def problem_of(case):
    return problem(DTYPE[case.dtype], case.K, case.structure, case.overlap)


@functools.lru_cache(maxsize=None)
def _want(oracle, pr, K, dtype, kw):
    return oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, dtype=dtype, nthreads=NT, **dict(kw))


def want(oracle, pr, K, dtype, **kw):
    """oracle.calc, once per (problem, keywords); the arrays are shared: nobody writes to them"""
    return _want(oracle, pr, K, dtype, tuple(sorted(kw.items())))


def want_of(oracle, case, **override):
    kw = plan.call_kw(case)
    kw.update(override)
    return want(oracle, problem_of(case), case.K, DTYPE[case.dtype], **kw)


@functools.lru_cache(maxsize=None)
def scores(oracle, pr, dtype):
    return oracle.scores(pr["A"], pr["B"], dtype=dtype)


def evaluated(pr, K, metrics, cold=True, min_items_pool=2, min_pos_test=1, **_):
    """per user: the eligibility rules say it is evaluated (oracle/recometrics_oracle.cpp eval_user and run, csrc/rm_prep.hpp k_classify)"""
    n = pr["B"].shape[0]
    ntr, npos = np.diff(pr["train"][0]), np.diff(pr["test"][0])
    pool, pos = max(min_items_pool, K, 2), min(min_pos_test, 1)
    out = (npos > 0) & ~((ntr + npos >= n) & ("ndcg" not in metrics)) & (n - ntr >= pool) & (cold | (ntr > 0)) & (npos >= pos)
    if not set(metrics) & {"roc", "pr", "ap", "tap", "rr"}:
        out &= n - ntr > K
    return out
