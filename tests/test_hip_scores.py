"""GPU: metrics from a caller's score matrix (rm_calc_metrics_scores_* / calc_reco_metrics_from_scores).

Three checkers:
 (a) the oracle on low-rank scores: S = oracle.scores(A, B) -- the k-ordered fma chain, bit-exact -- goes through the new entry and is
     compared with oracle.calc(A, B, noise off) the way tests/_parity.py compares: every metric bitwise, ROC-AUC (x87 long double in
     the reference, fp64 here) within an ulp of the output type (_util.roc_tol);
 (b) the factor call: the same S against rm_calc_metrics_* (noise off) on (A, B): all ten outputs bitwise, fp32 and fp64;
 (c) the oracle on free-form scores: oracle.calc(A = S, B = I) -- for finite S the chain returns S[u, i] exactly (and +0 for -0) --
     for scores that are no low-rank product.
"""
import functools
import os

import numpy as np
import pytest

from _parity import NT, hip_calc
from _requests import planted_problem, replace_rows
from _util import assert_roc, assert_same_bits

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ALL = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr")


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


# ---- the call ---------------------------------------------------------------------------------------------------------------------
def strided(S, pad):
    """S in a buffer whose rows are n + pad apart; with a pad the first row starts one element into the allocation (no row is
    16-byte aligned then) and everything between the rows is NaN"""
    m, n = S.shape
    ld = n + pad
    off = 1 if pad else 0
    buf = np.full(m * ld + off + 4, np.nan, S.dtype)
    V = buf[off:off + m * ld].reshape(m, ld)[:, :n]
    V[...] = S
    return V, ld


def scores_calc(hip, S, train, test, k, metrics=ALL, cumulative=False, cold=True, min_items_pool=2, min_pos_test=1, pad=0, dtype=F32, **_):
    from oracle.oracle import NAMES
    V, ld = strided(np.ascontiguousarray(S, dtype=dtype), pad)
    trp, tri = [np.ascontiguousarray(x, dtype=np.int32) for x in train[:2]]
    tep, tei = [np.ascontiguousarray(x, dtype=np.int32) for x in test[:2]]
    tev = np.ascontiguousarray(test[2], dtype=dtype) if len(test) > 2 and test[2] is not None else np.ones(tei.shape[0], dtype)
    want = {name: (name in metrics) for name in hip.METRIC_ORDER}
    keep = V.copy()
    outs = hip.calc_metrics_scores(V, ld, trp, tri, tep, tei, tev, k, want, cumulative, cold, min_items_pool, min_pos_test, 1)
    assert_same_bits(V, keep, "the caller's scores were modified")
    return {NAMES[name]: arr for name, arr in zip(hip.METRIC_ORDER, outs) if want[name]}


def assert_all_bits(got, want, what):
    assert set(got) == set(want), what
    for name in want:
        assert_same_bits(got[name], want[name], "%s: %s" % (what, name))


def assert_like_parity(got, want, what):
    """the comparison of tests/_parity.py `_check_against_oracle` with the restatement: bitwise, ROC-AUC within an ulp (roc_tol)"""
    assert set(got) == set(want), what
    for name in want:
        if name == "ROC_AUC":
            assert_roc(got[name], want[name], want[name].dtype, "%s: %s" % (what, name))
        else:
            assert_same_bits(got[name], want[name], "%s: %s (bitwise)" % (what, name))


# ---- problems ---------------------------------------------------------------------------------------------------------------------
# (replace_rows and planted_problem live in tests/_requests.py, which plants two more users into the same problem)


def run_a_and_b(hip, oracle, pr, K, dtype, pad, what, cumulative=(False, True), **kw):
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    for cum in cumulative:
        got = scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=cum, pad=pad, dtype=dtype, **kw)
        factor = hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, cumulative=cum, noise=False, dtype=dtype, **kw)
        assert_all_bits(got, factor, "%s cumulative=%s against the factor call" % (what, cum))
        want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K, cumulative=cum, noise=False, dtype=dtype, nthreads=NT, **kw)
        assert_like_parity(got, want, "%s cumulative=%s against the oracle" % (what, cum))
    return got


# ---- (a) + (b): shapes ------------------------------------------------------------------------------------------------------------
SHAPE_N = (1, 2, 63, 191, 192, 193, 1000, 4099)
SHAPE_CASES = [(n, pad, (1, 33, 129, 700)[(i + j) % 4], (1, 10, 100, 300, 0)[(2 * i + j) % 5])
               for i, n in enumerate(SHAPE_N) for j, pad in enumerate((0, 1, 3))]


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n,pad,m,K", SHAPE_CASES)
def test_shapes_against_the_oracle_and_the_factor_call(hip, oracle, dtype, n, pad, m, K):
    """item counts around the 64-item tiles and the 192-item padding, row strides n, n + 1, n + 3 (rows that are not 16-byte aligned),
    one user up to several blocks of users, K = 1 ... n, single and cumulative"""
    K = n if K == 0 else min(K, n)
    pr = planted_problem(m, n, 16, dtype, 100 + n, K)
    got = run_a_and_b(hip, oracle, pr, K, dtype, pad, "n=%d lds=n+%d m=%d K=%d" % (n, pad, m, K))
    if n >= 63 and m >= 33 and K < n // 2:
        assert np.isfinite(got["P@K"]).any(), "nobody was evaluated"


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [1, 10, 100, 300, 4099])
def test_every_k_with_the_planted_users(hip, oracle, dtype, K):
    """n = 4,099, 700 users, every K of the list with the users planted for it (C = K - 1, K, K + 1)"""
    pr = planted_problem(700, 4099, 16, dtype, 7, K)
    tep = pr["test"][0]
    assert list(np.diff(tep)[:6]) == [0, 1, 63, 64, 1023, 1500]
    run_a_and_b(hip, oracle, pr, K, dtype, 3, "planted users K=%d" % K)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("opts", [dict(cold=False), dict(min_pos_test=3), dict(min_items_pool=50), dict(cold=False, min_pos_test=3, min_items_pool=50)])
def test_eligibility_options(hip, oracle, dtype, opts):
    pr = planted_problem(129, 1000, 16, dtype, 11, 10)
    trp, tri = pr["train"]
    # some users without a train item (cold start)
    rows = {u: (np.zeros(0, np.int32), pr["test"][1][pr["test"][0][u]:pr["test"][0][u + 1]], None) for u in (20, 21, 22)}
    pr = replace_rows(pr, 1000, rows, dtype)
    run_a_and_b(hip, oracle, pr, 10, dtype, 1, "options %s" % opts, **opts)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("metrics", [("p",), ("ndcg",), ("roc",), ("pr",), ("hit", "rr"), ("ap", "tap", "roc")])
def test_subsets_of_the_metrics(hip, oracle, dtype, metrics):
    pr = planted_problem(129, 1000, 16, dtype, 12, 10)
    run_a_and_b(hip, oracle, pr, 10, dtype, 3, "metrics %s" % (metrics,), metrics=metrics)


# ---- (c): free-form scores ----------------------------------------------------------------------------------------------------------
def oracle_on_scores(oracle, S, train, test, K, dtype, **kw):
    """checker (c): A = S, B = I -- the chain adds S[u, i] * 1 to zeros"""
    n = S.shape[1]
    return oracle.calc(np.ascontiguousarray(S, dtype), np.eye(n, dtype=dtype), train, test, K, noise=False, dtype=dtype, nthreads=NT, **kw)


def check_free_form(hip, oracle, S, train, test, K, dtype, what, pad=1):
    assert np.isfinite(S).all()
    for cum in (False, True):
        got = scores_calc(hip, S, train, test, K, cumulative=cum, pad=pad, dtype=dtype)
        want = oracle_on_scores(oracle, S, train, test, K, dtype, cumulative=cum)
        assert_like_parity(got, want, "%s cumulative=%s" % (what, cum))
    return got


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [5, 40])
@pytest.mark.parametrize("kind", ["ascending", "descending", "trend", "planted", "outliers", "runs"])
def test_structured_scores_under_a_non_linear_head(hip, oracle, kind, K, dtype):
    """the structured kinds of synth.make_structured, pushed through a non-linear head (no low-rank product any more; monotone
    where it matters, so the order along the item axis survives; rounding makes exact ties)"""
    from recometrics_amd.synth import make_structured
    m, n = 200, 500
    pr = make_structured(kind, m, n, 8, dtype, mean_c=30, seed=5)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype).astype(np.float64)
    S = np.tanh(S / (1.0 + np.abs(S).mean())) + 0.25 * np.sin(3.0 * S)
    if kind == "runs":
        S = np.round(S * 64) / 64
    got = check_free_form(hip, oracle, S.astype(dtype), pr["train"], pr["test"], K, dtype, kind)
    assert np.isfinite(got["P@K"]).sum() > m // 2


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [1, 10])
def test_all_scores_equal(hip, oracle, dtype, K):
    """every candidate the same score: invalid for everybody (the validity rule), as the oracle says"""
    pr = planted_problem(129, 500, 16, dtype, 13, K)
    S = np.full((129, 500), 0.75, dtype)
    got = check_free_form(hip, oracle, S, pr["train"], pr["test"], K, dtype, "all equal")
    assert np.isnan(got["P@K"]).all()
    # ... and equal but for one item per user: ordered by item id
    S[np.arange(129), np.arange(129) * 3 % 500] = 1.5
    check_free_form(hip, oracle, S, pr["train"], pr["test"], K, dtype, "all equal but one")


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [1, 10, 100])
def test_exact_ties_across_the_kth_place(hip, oracle, dtype, K):
    """scores on a grid of a few values: ties inside the list, across its edge, and between positives and candidates"""
    pr = planted_problem(256, 512, 16, dtype, 14, K)
    rng = np.random.default_rng(14)
    S = (rng.integers(-6, 7, size=(256, 512)) / 4.0).astype(dtype)
    check_free_form(hip, oracle, S, pr["train"], pr["test"], K, dtype, "ties", pad=3)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [1, 10])
def test_positive_and_negative_zero_are_the_same_score(hip, oracle, dtype, K):
    pr = planted_problem(256, 512, 16, dtype, 15, K)
    rng = np.random.default_rng(15)
    S = (rng.integers(-2, 3, size=(256, 512)) / 2.0).astype(dtype)
    S[(S == 0) & (rng.random(S.shape) < 0.5)] = -0.0
    assert np.signbit(S[S == 0]).any() and not np.signbit(S[S == 0]).all()
    got = check_free_form(hip, oracle, S, pr["train"], pr["test"], K, dtype, "signed zeros")
    plus = scores_calc(hip, np.where(S == 0, 0.0, S).astype(dtype), pr["train"], pr["test"], K, cumulative=True, dtype=dtype)
    assert_all_bits(got, plus, "-0 against +0")


# ---- non-finite scores ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def poison_problem(dtype):
    from recometrics_amd.synth import make_problem
    pr = make_problem(300, 5000, 64, dtype, mean_c=40, seed=1064)
    item = 1234
    trp, tri = pr["train"]
    tep, tei, tev = pr["test"]
    has = np.array([item in tri[trp[u]:trp[u + 1]] for u in range(300)])
    rows = {}
    for u in (11, 12, 13):                                  # somebody with an ordinary row has the item in its train row
        if not has[u]:
            te = tei[tep[u]:tep[u + 1]]
            rows[u] = (np.union1d(tri[trp[u]:trp[u + 1]], [item]).astype(np.int32), te[te != item], tev[tep[u]:tep[u + 1]][te != item])
    pr = replace_rows(pr, 5000, rows, dtype)
    trp, tri = pr["train"]
    has = np.array([item in tri[trp[u]:trp[u + 1]] for u in range(300)])
    return pr, item, has


@pytest.mark.parametrize("dtype,K", [(F32, 10), (F64, 10), (F32, 300)])
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_non_finite_column(hip, oracle, dtype, K, poison):
    """a column of NaN / +Inf / -Inf: a user with the item in its TRAIN row is unchanged bit for bit; a user for whom it is a candidate
    is NaN everywhere for a NaN (D3) and follows the factor call's validity rule for an infinity (the factor call and the oracle on an
    item whose factors give exactly these scores)"""
    pr, item, has = poison_problem(dtype)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    clean = scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=True, dtype=dtype)
    P = S.copy()
    P[:, item] = poison
    got = scores_calc(hip, P, pr["train"], pr["test"], K, cumulative=True, pad=1, dtype=dtype)
    assert has[11] and has.sum() >= 3
    for name in clean:
        assert_same_bits(got[name][has], clean[name][has], "%s of the users that mask the item" % name)
        if poison != poison:
            assert np.isnan(got[name][~has]).all(), name
    if poison == poison:
        # the validity rule: an item row that scores `poison` for every user, through the factor call and the oracle
        # (one-hot factors: the chain adds poison * 1 to zeros in the last place -- and only there, so nothing else turns NaN)
        A1 = np.hstack([pr["A"], np.ones((300, 1), dtype)])
        B1 = np.hstack([pr["B"], np.zeros((5000, 1), dtype)])
        B1[item, :] = 0
        B1[item, -1] = poison
        S1 = oracle.scores(A1, B1, dtype=dtype)
        assert_same_bits(S1[:, item], P[:, item], "the poisoned column")
        keep = np.arange(5000) != item
        assert_same_bits(S1[:, keep], P[:, keep], "the other columns")
        factor = hip_calc(hip, A1, B1, pr["train"], pr["test"], K, cumulative=True, noise=False, dtype=dtype)
        assert_all_bits(got, factor, "an infinite column against the factor call")
        want = oracle.calc(A1, B1, pr["train"], pr["test"], K, cumulative=True, noise=False, dtype=dtype, nthreads=NT)
        assert_like_parity(got, want, "an infinite column against the oracle")
        if poison > 0:
            assert np.isnan(got["P@K"][~has]).all()          # (an infinite best score)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("garbage", [np.nan, np.inf, -np.inf])
def test_scores_at_train_items_are_never_looked_at(hip, oracle, dtype, garbage):
    pr = planted_problem(129, 1000, 16, dtype, 16, 10)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    clean = scores_calc(hip, S, pr["train"], pr["test"], 10, cumulative=True, dtype=dtype)
    trp, tri = pr["train"]
    G = S.copy()
    G[np.repeat(np.arange(129), np.diff(trp)), tri] = garbage
    assert not np.isfinite(G).all()
    got = scores_calc(hip, G, pr["train"], pr["test"], 10, cumulative=True, pad=3, dtype=dtype)
    assert_all_bits(got, clean, "garbage at the train positions")


# ---- CSR handling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F64, 100)])
def test_unsorted_rows_and_bad_indices(hip, oracle, dtype, K):
    pr = planted_problem(300, 4099, 16, dtype, 17, K)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    trp, tri = pr["train"]
    want = scores_calc(hip, S, pr["train"], pr["test"], K, dtype=dtype)
    rng = np.random.default_rng(3)
    shuffled = tri.copy()
    for u in range(0, 300, 3):
        shuffled[trp[u]:trp[u + 1]] = rng.permutation(shuffled[trp[u]:trp[u + 1]])
    assert (shuffled != tri).any()
    keep = shuffled.copy()
    assert_all_bits(scores_calc(hip, S, (trp, shuffled), pr["test"], K, dtype=dtype), want, "unsorted train rows")
    assert (shuffled == keep).all(), "the caller's arrays were modified"
    tep, tei, tev = pr["test"]
    te_shuffled, tv_shuffled = tei.copy(), tev.copy()
    for u in range(1, 300, 3):
        o = rng.permutation(tep[u + 1] - tep[u])
        te_shuffled[tep[u]:tep[u + 1]] = tei[tep[u]:tep[u + 1]][o]
        tv_shuffled[tep[u]:tep[u + 1]] = tev[tep[u]:tep[u + 1]][o]
    assert_all_bits(scores_calc(hip, S, (trp, shuffled), (tep, te_shuffled, tv_shuffled), K, dtype=dtype), want, "unsorted train and test rows")
    bad = tri.copy()
    bad[trp[17]] = 4099
    with pytest.raises(ValueError, match="row 17"):
        scores_calc(hip, S, (trp, bad), pr["test"], K, dtype=dtype)
    bad_te = tei.copy()
    bad_te[tep[23]] = -1
    with pytest.raises(ValueError, match="row 23"):
        scores_calc(hip, S, pr["train"], (tep, bad_te, tev), K, dtype=dtype)
    assert_all_bits(scores_calc(hip, S, pr["train"], pr["test"], K, dtype=dtype), want, "after the errors")


# ---- one mid-size case ------------------------------------------------------------------------------------------------------------
def test_c2_item_count_2048_users(hip, oracle):
    """2,048 users x 26,744 items (BASELINE C2's item count: 219 MB of scores), fp32, K = 10, checkers (a) and (b)"""
    from recometrics_amd.synth import make_factors, make_interactions_fast
    m, n, kf = 2048, 26744, 64
    A, B = make_factors(m, n, kf, F32, 2)
    trp, tri, tep, tei, tev = make_interactions_fast(m, n, 100, F32, 2)
    pr = dict(A=A, B=B, train=(trp, tri), test=(tep, tei, tev))
    assert np.diff(tep).max() > 63
    got = run_a_and_b(hip, oracle, pr, 10, F32, 0, "C2's item count", cumulative=(False,))
    assert np.isfinite(got["ROC_AUC"]).sum() > 2000


# ---- entry points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 300), (F64, 10)])
def test_shards_and_batches_change_nothing(hip, monkeypatch, oracle, dtype, K):
    m, n = 3000, 1000
    pr = planted_problem(m, n, 16, dtype, 18, K)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    plain = scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=True, pad=1, dtype=dtype)
    hip.set_devices([0, 0])
    try:
        assert_all_bits(scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=True, pad=1, dtype=dtype), plain, "two shards")
    finally:
        hip.set_devices([])
    monkeypatch.setenv("RM_BATCH_USERS", "700")
    assert_all_bits(scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=True, pad=1, dtype=dtype), plain, "batches of 700 users")
    hip.set_devices([0, 0])
    try:
        assert_all_bits(scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=True, pad=1, dtype=dtype), plain, "two shards in batches")
    finally:
        hip.set_devices([])


_DEVICE_ENTRY_SCRIPT = r"""
import json, os, sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch                                           # (before the library: the order bench.py loads them in)
from recometrics_amd import _binding as hip
from oracle.oracle import Oracle
from test_hip_scores import planted_problem, scores_calc, ALL
from _util import assert_same_bits
torch.cuda.set_device(0); hip.load(); hip.set_device(0)
dev = torch.device("cuda", 0)
side = torch.cuda.Stream(device=dev)                   # a stream that is not the default one
oracle = Oracle()
m, n = 300, 4099
done = []
for dtype, K, cum in ((np.float32, 10, False), (np.float32, 300, True), (np.float64, 10, True)):
    pr = planted_problem(m, n, 16, dtype, 19, K)
    S = oracle.scores(pr["A"], pr["B"], dtype=dtype)
    want = scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=cum, dtype=dtype)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    ld = n + 3
    wide = torch.full((m * ld + 1,), float("nan"), dtype=tdt, device=dev)
    view = wide[1:].view(m, ld)[:, :n]
    view.copy_(torch.from_numpy(S).to(dev))
    trp, tri = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev) for x in pr["train"]]
    tep, tei = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev) for x in pr["test"][:2]]
    tev = torch.from_numpy(np.ascontiguousarray(pr["test"][2], dtype)).to(dev)
    from oracle.oracle import NAMES
    outs = [torch.full((m, K) if (cum and i < 8) else (m,), 7.0, dtype=tdt, device=dev) for i in range(10)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hip.calc_metrics_scores_device(dtype, view.data_ptr(), ld, m, n, trp.data_ptr(), tri.data_ptr(), int(tri.shape[0]),
                                       tep.data_ptr(), tei.data_ptr(), tev.data_ptr(), int(tei.shape[0]), K,
                                       [o.data_ptr() for o in outs], cumulative=cum, stream=side.cuda_stream)
    side.synchronize()
    for name, o in zip(hip.METRIC_ORDER, outs):
        assert_same_bits(o.cpu().numpy(), want[NAMES[name]], "device entry: " + name)
    tm = hip.timings()
    assert tm["device_ms"] > 0 and tm["sweep_ms"] > 0 and tm["finalize_ms"] > 0 and tm["sweep_blocks"] > 0, tm
    done.append([np.dtype(dtype).name, K])
# the working rows of m users do not fit: RM_ERR_NOMEM with the bytes per row and the largest m that fits
hip.load().rm_release_workspace()
os.environ["RM_DEBUG_FREE_MB"] = "8"
hip.reload_switches()
try:
    hip.calc_metrics_scores_device(dtype, view.data_ptr(), ld, m, n, trp.data_ptr(), tri.data_ptr(), int(tri.shape[0]),
                                   tep.data_ptr(), tei.data_ptr(), tev.data_ptr(), int(tei.shape[0]), K,
                                   [o.data_ptr() for o in outs], cumulative=cum, stream=side.cuda_stream)
    raise SystemExit("no MemoryError")
except MemoryError as e:
    msg = str(e)
row_bytes = (n + 191) // 192 * 192 * 8
assert "score matrix" in msg and "(%%d B) per user" %% row_bytes in msg and "%%d users do not fit" %% m in msg and "at most" in msg, msg
most = int(msg.split("at most ")[1].split()[0])
assert 0 < most < m, msg
del os.environ["RM_DEBUG_FREE_MB"]
hip.reload_switches()
torch.cuda.synchronize()
print(json.dumps(done + [most]))
"""


def test_device_entry(hip):
    """torch device tensors in (a row stride of n + 3, no row 16-byte aligned), metrics in device tensors out on a stream that is not
    the default one, equal to the host entry's bit for bit; rm_get_timings; RM_ERR_NOMEM with its message under a simulated small
    device.  (A process of its own: the tensors are torch's, and torch wants to be loaded before the library.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _DEVICE_ENTRY_SCRIPT % {"root": root}], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert len(json.loads(res.stdout.strip().splitlines()[-1])) == 4


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_calc_reco_metrics_from_scores(hip, oracle, dtype):
    from scipy.sparse import csr_array
    from recometrics_amd import calc_reco_metrics, calc_reco_metrics_from_scores
    m, n, K = 300, 1000, 7
    pr = planted_problem(m, n, 16, dtype, 20, K)
    A, B = pr["A"], pr["B"]
    S = oracle.scores(A, B, dtype=dtype)
    trp, tri = pr["train"]
    tep, tei, tev = pr["test"]
    X_train = csr_array((np.ones(tri.shape[0], dtype), tri, trp), shape=(m, n))
    X_test = csr_array((tev, tei, tep), shape=(m, n))
    # (the row of user 0 has no test item: fine -- but X_test must hold something)
    want = calc_reco_metrics(X_train, X_test, A, B, k=K, all_metrics=True, break_ties_with_noise=False)
    got = calc_reco_metrics_from_scores(X_train, X_test, S, k=K, all_metrics=True)
    assert list(got.columns) == list(want.columns) and got.shape == want.shape
    assert got.values.dtype == dtype and got.values.flags["F_CONTIGUOUS"]
    assert_same_bits(got.values, want.values, "frame values")
    d_want = calc_reco_metrics(X_train, X_test, A, B, k=K, as_df=False, break_ties_with_noise=False)
    d_got = calc_reco_metrics_from_scores(X_train, X_test, S, k=K, as_df=False)
    assert set(d_got) == set(d_want) and d_got["K"] == K
    for key in d_want:
        if key != "K":
            assert_same_bits(d_got[key], d_want[key], key)
    c_want = calc_reco_metrics(X_train, X_test, A, B, k=K, all_metrics=True, cumulative=True, break_ties_with_noise=False)
    c_got = calc_reco_metrics_from_scores(X_train, X_test, S, k=K, all_metrics=True, cumulative=True)
    assert list(c_got.columns) == list(c_want.columns)
    assert_same_bits(c_got.values, c_want.values, "cumulative frame")
    n_want = calc_reco_metrics(None, X_test, A, B, k=K, all_metrics=True, break_ties_with_noise=False, consider_cold_start=False)
    n_got = calc_reco_metrics_from_scores(None, X_test, S, k=K, all_metrics=True, consider_cold_start=False)
    assert_same_bits(n_got.values, n_want.values, "X_train=None")
    assert not n_got.equals(got)
    fort = np.asfortranarray(S)
    assert_same_bits(calc_reco_metrics_from_scores(X_train, X_test, fort, k=K, all_metrics=True).values, want.values, "Fortran-ordered scores")
    wide = np.full((m, n + 5), np.nan, dtype)
    wide[:, 2:2 + n] = S
    assert_same_bits(calc_reco_metrics_from_scores(X_train, X_test, wide[:, 2:2 + n], k=K, all_metrics=True).values, want.values, "strided scores")
    if dtype == F32:                                   # anything but float32 is evaluated in float64
        w64 = calc_reco_metrics_from_scores(X_train, X_test, S.astype(np.float64), k=K, all_metrics=True)
        assert w64.values.dtype == np.float64 and (np.isnan(w64.values) == np.isnan(want.values)).all()
