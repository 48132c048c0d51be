"""GPU: metric requests WITHOUT ROC-AUC -- above all the call with every keyword at its default (precision, average precision, NDCG,
tie noise on) -- against the oracle bit for bit, the compiled reference where it is built, and the all-ten call on the same inputs.

Such a request takes another road on the device at almost every stage: k_classify decides who is evaluated from the request
(UF_ONLY_NDCG, UF_KLEQN), there are no positives' tables, chunks or streamed users (one slot per user, however long its test row),
the sweep keeps longer lists in LDS, k_finalize applies the partial validity rule (best score == K-th score), is the only kernel
that flags users for the exact pass of the fp32 tie noise, and walks long test rows on one thread.  The problems are built so that
each of these decides the outputs of many users (tests/_requests.py; tests/test_requests_cpu.py asserts that they do); the checker
is _requests.check_request."""
import inspect

import numpy as np
import pytest

from _parity import NT, hip_calc
from _requests import (DEFAULT, F32, F64, REQUESTS, TIE_REQUESTS, TOPK8, check_request, edge_problem, equal_problem,
                       long_rows_problem, req_id, runs_problem, tie_problem, user_is_nan)
from _util import assert_roc, assert_same_bits
from test_hip_scores import scores_calc

pytestmark = pytest.mark.gpu
# ("p", "roc") has the all-ten call's NaN pattern for every planted user at every K (test_requests_cpu): not run on the edge users
EDGE_REQUESTS = tuple(req for req in REQUESTS if req != ("p", "roc"))
NOISE_REQUESTS = (DEFAULT, TOPK8, ("p",))
SEEDS = (2 ** 33 + 5, 1)
dtype_id = lambda d: np.dtype(d).name


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


def set_env(monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)


# ---- 1. eligibility by request: k_classify, the NaN overrides of k_finalize ------------------------------------------------------------
@pytest.mark.parametrize("req", EDGE_REQUESTS, ids=req_id)
@pytest.mark.parametrize("K", [1, 10, 100])
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_edge_users(hip, oracle, dtype, K, req):
    check_request(hip, oracle, edge_problem(dtype, K), K, dtype, req)


@pytest.mark.parametrize("req", [DEFAULT, TOPK8], ids=req_id)
@pytest.mark.parametrize("K", [1, 10, 100])
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_edge_users_with_tie_noise(hip, oracle, dtype, K, req):
    check_request(hip, oracle, edge_problem(dtype, K), K, dtype, req, noise=True, seed=7)


@pytest.mark.parametrize("req", EDGE_REQUESTS, ids=req_id)
@pytest.mark.parametrize("opts", [dict(cold=False), dict(min_pos_test=3), dict(min_items_pool=50), dict(cold=False, min_pos_test=3, min_items_pool=50)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_edge_users_under_the_eligibility_options(hip, oracle, dtype, opts, req):
    check_request(hip, oracle, edge_problem(dtype, 10, cold_rows=True), 10, dtype, req, **opts)


# ---- 2. the partial validity rule under exact ties, through every producer of the K-th entry -----------------------------------------
TIE_CASES = (
    [({}, dtype, K) for dtype, K in ((F32, 10), (F32, 20), (F32, 100), (F32, 300), (F64, 10), (F64, 100), (F64, 300))]
    + [({"RM_DEBUG_HBM_LISTS": "1"}, F32, 20), ({"RM_DEBUG_HBM_LISTS": "1", "RM_DEBUG_LANE_MIN_K": "1000000"}, F64, 12)]
    + [({"RM_DEBUG_LANE_CAP_MIN": "1"}, F32, 33), ({"RM_DEBUG_LANE_CAP_MIN": "1"}, F64, 50)]
    + [({"RM_DEBUG_LANE_MIN_K": "1"}, F32, 3), ({"RM_DEBUG_EXT_TOPK": "1"}, F32, 10)]
    + [({"RM_DEBUG_SPLITS": "3,2,5"}, F32, 10), ({"RM_DEBUG_SPLITS": "3,2,5"}, F32, 100), ({"RM_DEBUG_SPLITS": "3,2,5"}, F64, 50)]
    + [({"RM_DEBUG_NSUB2": "1"}, F32, 10), ({"RM_DEBUG_NO_TRAIN_BITS": "1"}, F32, 10)]
    + [({"RM_DEBUG_SAMPLE_SEED": "64"}, F32, 12), ({"RM_DEBUG_SAMPLE_SEED": "64"}, F32, 100), ({"RM_DEBUG_NO_SEED": "1"}, F32, 100)]
)


def case_id(case):
    env, dtype, K = case
    return "-".join(["%s=%s" % (k[3:].replace("DEBUG_", ""), v) for k, v in env.items()] + [dtype_id(dtype), "K%d" % K])


@pytest.mark.parametrize("req", TIE_REQUESTS, ids=req_id)
@pytest.mark.parametrize("case", TIE_CASES, ids=case_id)
def test_tied_zeros_at_the_top(hip, oracle, monkeypatch, case, req):
    """a third of the users have ~750 exactly tied zeros at the top of their ranking: NaN without ROC-AUC, valid with it"""
    env, dtype, K = case
    set_env(monkeypatch, env)
    got = check_request(hip, oracle, tie_problem(dtype), K, dtype, req)
    dead = user_is_nan(got)
    assert (not dead.any()) if "roc" in req else (dead.sum() >= 100 and dead[::3].all())


@pytest.mark.parametrize("req", TIE_REQUESTS, ids=req_id)
@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_runs_of_equal_scores(hip, oracle, dtype, K, req):
    """the ramp in runs of about 40 equal scores: K = 10 inside the best run (NaN without ROC-AUC), K = 100 beyond it"""
    got = check_request(hip, oracle, runs_problem(dtype), K, dtype, req)
    dead = user_is_nan(got)
    assert dead.sum() >= 100 if (K == 10 and "roc" not in req) else not dead.any()


@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_all_scores_equal(hip, oracle, dtype):
    for req in TIE_REQUESTS:
        assert user_is_nan(check_request(hip, oracle, equal_problem(dtype), 10, dtype, req)).all(), req
    assert user_is_nan(check_request(hip, oracle, equal_problem(dtype), 10, dtype, DEFAULT, noise=True, seed=3)).all()


# ---- 3. tie noise without the AUCs: flags from k_finalize only, the exact pass ------------------------------------------------------
NOISE_CASES = ([({}, dtype, K) for dtype in (F32, F64) for K in (10, 100, 300)]
               + [({"RM_NOISE_BUDGET_MB": "1"}, F32, 10), ({"RM_DEBUG_SPLITS": "3,2,5"}, F32, 10), ({"RM_DEBUG_NO_SIDE": "1"}, F32, 10)])


@pytest.mark.parametrize("req", NOISE_REQUESTS, ids=req_id)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", NOISE_CASES, ids=case_id)
def test_tie_noise_orders_the_tied_zeros(hip, oracle, monkeypatch, case, seed, req):
    """the same users, noise on: only the noise orders their lists; bitwise the oracle's (fp64: and the compiled reference's)"""
    env, dtype, K = case
    set_env(monkeypatch, env)
    got = check_request(hip, oracle, tie_problem(dtype), K, dtype, req, noise=True, seed=seed)
    assert not user_is_nan(got).any()


def test_tie_noise_in_batches_and_shards(hip, oracle, monkeypatch):
    """the host entry: 2,600 users in batches of 1,500, on two shards, and both -- the bits of the single call and of the oracle"""
    pr = tie_problem(F32, 2600, 2000, 16)
    for noise in (True, False):
        kw = dict(metrics=DEFAULT, noise=noise, seed=SEEDS[0], cumulative=True)
        want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], 10, dtype=F32, nthreads=NT, **kw)

        def run(what):
            got = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], 10, **kw)
            assert set(got) == set(want)
            for name in want:
                assert_same_bits(got[name], want[name], "%s noise=%s: %s" % (what, noise, name))
        run("one call")
        monkeypatch.setenv("RM_BATCH_USERS", "1500")
        run("batches of 1,500 users")
        monkeypatch.delenv("RM_BATCH_USERS")
        hip.set_devices([0, 0])
        try:
            run("two shards")
            monkeypatch.setenv("RM_BATCH_USERS", "1500")
            run("two shards in batches of 1,500 users")
        finally:
            hip.set_devices([])
        monkeypatch.delenv("RM_BATCH_USERS")


# ---- 4. long test rows on one thread of k_finalize ---------------------------------------------------------------------------------
@pytest.mark.parametrize("req", [("ndcg",), DEFAULT, TOPK8], ids=req_id)
@pytest.mark.parametrize("K", [10, 65, 100, 256])
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_long_test_rows(hip, oracle, dtype, K, req):
    """test rows of 1 ... 4,000 items: nobody is streamed or chunked without the AUCs; the ideal DCG beyond the finalize buffer"""
    check_request(hip, oracle, long_rows_problem(dtype), K, dtype, req)


@pytest.mark.parametrize("req", [("ndcg",), DEFAULT, TOPK8], ids=req_id)
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_long_test_rows_with_tie_noise(hip, oracle, dtype, req):
    check_request(hip, oracle, long_rows_problem(dtype), 10, dtype, req, noise=True, seed=9)


# ---- 5. the call as typed, and the score-matrix entry --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_the_call_as_typed(hip, oracle, dtype):
    """calc_reco_metrics(X_train, X_test, A, B) and nothing else"""
    from scipy.sparse import csr_array
    import recometrics_amd
    par = inspect.signature(recometrics_amd.calc_reco_metrics).parameters
    k, seed = par["k"].default, par["seed"].default
    pr = tie_problem(dtype)
    m, n = 300, 5000
    trp, tri = pr["train"]
    tep, tei, tev = pr["test"]
    X_train = csr_array((np.ones(tri.shape[0], dtype), tri, trp), shape=(m, n))
    X_test = csr_array((tev, tei, tep), shape=(m, n))
    df = recometrics_amd.calc_reco_metrics(X_train, X_test, pr["A"], pr["B"])
    want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], k, metrics=DEFAULT, noise=True, seed=seed, dtype=dtype, nthreads=NT)
    assert list(df.columns) == ["P@%d" % k, "AP@%d" % k, "NDCG@%d" % k] and df.shape == (m, 3)
    assert df.values.dtype == dtype and all(t == dtype for t in df.dtypes)
    for col, name in zip(df.columns, ("P@K", "AP@K", "NDCG@K")):
        assert_same_bits(df[col].to_numpy(), want[name], "the default call: " + col)
    assert np.isfinite(df.values).all()
    out = recometrics_amd.calc_reco_metrics(X_train, X_test, pr["A"], pr["B"], as_df=False, cumulative=True)
    want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], k, metrics=DEFAULT, cumulative=True, noise=True, seed=seed, dtype=dtype, nthreads=NT)
    assert set(out) == {"P@K", "AP@K", "NDCG@K", "K"} and out["K"] == k
    for name in want:
        assert out[name].dtype == dtype and out[name].shape == (m, k)
        assert_same_bits(out[name], want[name], "the default call, cumulative: " + name)


@pytest.mark.parametrize("req", [DEFAULT, ("pr",), ("p", "roc")], ids=req_id)
@pytest.mark.parametrize("K", [10, 300])
@pytest.mark.parametrize("dtype", [F32, F64], ids=dtype_id)
def test_the_score_matrix_entry(hip, oracle, dtype, K, req):
    """S = oracle.scores(A, B) of the tie problem through calc_metrics_scores: the factor call's bits (noise off) and the oracle's"""
    pr = tie_problem(dtype)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    for cum in (False, True):
        got = scores_calc(hip, S, pr["train"], pr["test"], K, metrics=req, cumulative=cum, pad=1, dtype=dtype)
        factor = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, cumulative=cum, noise=False, dtype=dtype)
        want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=req, cumulative=cum, noise=False, dtype=dtype, nthreads=NT)
        assert set(got) == set(factor) == set(want) and len(got) == len(req)
        for name in want:
            assert_same_bits(got[name], factor[name], "%s cumulative=%s against the factor call" % (name, cum))
            if name == "ROC_AUC":
                assert_roc(got[name], want[name], dtype, name)
            else:
                assert_same_bits(got[name], want[name], "%s cumulative=%s against the oracle" % (name, cum))
        dead = user_is_nan(got)
        assert (not dead.any()) if "roc" in req else (dead.sum() >= 100 and dead[::3].all())
