"""GPU: the recommendation lists (rm_recommend_* / recommend_topk) against the oracle restatement.

The compiled reference has no list output, so the expected values come from the restatement (pinned to the reference by
tests/test_oracle_golden.py), two ways:

 (1) PRIMARY, every user: S = oracle.scores(A, B) -- the k-ordered fma chain, bit-exact -- then per user the items outside its row
     ordered by (score descending, item id ascending); status 1 for an empty candidate set, 2 when a candidate score is not finite.
     Ids equal, scores equal in every bit, status equal.
 (2) CROSS-CHECK: oracle.rank -- the ranking the metric parity rests on -- with a dummy test matrix of one item per user (the smallest
     id outside its row), min_items_pool = 1, cold start on, noise off: every user it ranks (status 0) must have the same list, bit
     for bit.  It cannot rank users with fewer than max(K, 2) candidates or all-equal scores; the i.i.d. cases assert that it covered
     at least 95 % of their users, so that it cannot pass by ranking nobody.
"""
import functools

import numpy as np
import pytest

from _util import assert_same_bits

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


# ---- the two checkers -------------------------------------------------------------------------------------------------------------
def expected_lists(S, excl, K, users=None):
    """checker (1) on the score matrix S [len(users) or m, n]; excl = (indptr, indices) or None"""
    rows = np.arange(S.shape[0]) if users is None else np.asarray(users)
    n = S.shape[1]
    ids = np.full((rows.shape[0], K), -1, np.int32)
    sc = np.full((rows.shape[0], K), np.nan, S.dtype)
    st = np.zeros(rows.shape[0], np.int32)
    for r, u in enumerate(rows):
        keep = np.ones(n, bool)
        if excl is not None:
            keep[excl[1][excl[0][u]:excl[0][u + 1]]] = False
        cand = np.flatnonzero(keep)
        if cand.shape[0] == 0:
            st[r] = 1
            continue
        s = S[r, cand]
        if not np.isfinite(s).all():
            st[r] = 2
            continue
        o = np.lexsort((cand, -s))[:K]
        ids[r, :o.shape[0]] = cand[o]
        sc[r, :o.shape[0]] = s[o]
    return ids, sc, st


def check_lists(got, want, what=""):
    ids, sc, st = got
    wids, wsc, wst = want
    assert (st == wst).all(), "%s: status differs for users %s (got %s, want %s)" % (
        what, np.flatnonzero(st != wst)[:8].tolist(), st[st != wst][:8].tolist(), wst[st != wst][:8].tolist())
    bad = np.flatnonzero((ids != wids).any(axis=1))
    assert bad.shape[0] == 0, "%s: ids differ for %d users, e.g. user %d: got %s want %s" % (
        what, bad.shape[0], bad[0], ids[bad[0]][:12].tolist(), wids[bad[0]][:12].tolist())
    if sc is not None:
        assert_same_bits(sc, wsc, what + " scores")


def cross_check_with_oracle_rank(oracle, A, B, excl, K, got, dtype, min_coverage=None, what=""):
    """checker (2); returns the number of users oracle.rank ranked"""
    m, n = A.shape[0], B.shape[0]
    p, i = excl
    tep = np.zeros(m + 1, np.int64)
    tei = []
    for u in range(m):
        keep = np.ones(n, bool)
        keep[i[p[u]:p[u + 1]]] = False
        first = np.flatnonzero(keep)[:1]
        tei.append(first)
        tep[u + 1] = tep[u] + first.shape[0]
    tei = np.concatenate(tei).astype(np.int32)
    tep = tep.astype(np.int32)
    rk = oracle.rank(A, B, (p, i), (tep, tei, None), K, noise=False, cold=True, min_items_pool=1, min_pos_test=1, dtype=dtype)
    ranked = np.flatnonzero(rk["status"] == 0)
    ids, sc, st = got
    assert (st[ranked] == 0).all(), what
    assert (ids[ranked] == rk["topk_idx"][ranked]).all(), what + ": ids differ from oracle.rank"
    assert_same_bits(sc[ranked], rk["topk_score"][ranked], what + " scores against oracle.rank")
    if min_coverage is not None:
        assert ranked.shape[0] >= min_coverage * m, "%s: oracle.rank ranked only %d of %d users" % (what, ranked.shape[0], m)
    return ranked.shape[0]


# ---- problems ---------------------------------------------------------------------------------------------------------------------
def plant_rows(excl, n, rows):
    """the exclusion matrix with the rows of `rows` = {user: number of CANDIDATES} replaced: the row excludes all items but that many
    (spread over the whole id range: the first and the last item are candidates when there are two or more)"""
    p, i = excl
    m = p.shape[0] - 1
    out = []
    for u in range(m):
        if u in rows:
            c = rows[u]
            keep = np.unique(np.round(np.linspace(0, n - 1, c)).astype(np.int64)) if c > 0 else np.zeros(0, np.int64)
            assert keep.shape[0] == c
            mask = np.ones(n, bool)
            mask[keep] = False
            out.append(np.flatnonzero(mask).astype(np.int32))
        else:
            out.append(i[p[u]:p[u + 1]])
    q = np.zeros(m + 1, np.int64)
    np.cumsum([x.shape[0] for x in out], out=q[1:])
    return q.astype(np.int32), np.concatenate(out).astype(np.int32)


@functools.lru_cache(maxsize=8)
def iid_problem(m, n, kf, dtype, seed, quarters=False):
    """i.i.d. factors, make_interactions(mean 40) train rows, plus three planted users: empty row, full row, all but three items"""
    from recometrics_amd.synth import make_factors, make_interactions
    A, B = make_factors(m, n, kf, dtype, seed)
    if quarters:                                     # exact ties inside the lists and across their edge
        A, B = (np.round(A * 8) / 4).astype(dtype), (np.round(B * 8) / 4).astype(dtype)
    trp, tri = make_interactions(m, n, 40, dtype, seed)[:2]
    excl = plant_rows((trp, tri), n, {1: n, m // 2: 0, m - 2: 3})
    return A, B, excl


def run_host(hip, A, B, excl, K, scores=True):
    return hip.recommend(A, A.shape[1], B, B.shape[1], None if excl is None else excl[0], None if excl is None else excl[1], K, scores)


def check_problem(hip, oracle, A, B, excl, K, dtype, what, min_coverage=None, cross=True):
    got = run_host(hip, A, B, excl, K)
    S = oracle.scores(A, B, dtype=dtype)
    check_lists(got, expected_lists(S, excl, K), what)
    if cross and excl is not None:
        cross_check_with_oracle_rank(oracle, A, B, excl, K, got, dtype, min_coverage, what)
    return got


# ---- i.i.d. factors: both precisions, the kernel families' factor counts, K on both sides of every list-scheme boundary ------------
# fp32 lists: LDS replace-the-minimum below 20 (up to 64 factors: three sub-tiles) / below 14 (beyond), lane buffers + k_collect_topk
# up to 1,354 (k_collect_topk's three LDS sizes: K <= 128, <= 512, beyond), score rows + k_select_topk beyond; fp64: lane buffers at
# every K up to 1,354
_IID = [(F32, 8, 1), (F32, 50, 10), (F32, 64, 13), (F32, 64, 14), (F32, 64, 19), (F32, 64, 20), (F32, 128, 13), (F32, 128, 14),
        (F32, 128, 100), (F32, 200, 256), (F32, 300, 300), (F32, 64, 600),
        (F64, 8, 1), (F64, 50, 10), (F64, 64, 20), (F64, 128, 100), (F64, 200, 256), (F64, 300, 300)]


@pytest.mark.parametrize("dtype,kf,K", _IID, ids=["%s-k%d-K%d" % (np.dtype(a).name, b, c) for a, b, c in _IID])
def test_iid_factors(hip, oracle, dtype, kf, K):
    A, B, excl = iid_problem(300, 5000, kf, dtype, 1000 + kf)
    check_problem(hip, oracle, A, B, excl, K, dtype, "iid", min_coverage=0.95)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_k_beyond_the_lane_buffers_and_k_equal_n(hip, oracle, dtype):
    """K > 1,354: every user keeps a score row, k_select_topk; then K == n (every user has fewer candidates than K, or exactly K)"""
    A, B, excl = iid_problem(96, 2000, 64, dtype, 7)
    check_problem(hip, oracle, A, B, excl, 1500, dtype, "K=1500", min_coverage=0.95)
    A, B, excl = iid_problem(64, 300, 64, dtype, 8)
    check_problem(hip, oracle, A, B, excl, 300, dtype, "K=n")              # (oracle.rank ranks next to nobody here: no coverage asked)


@pytest.mark.parametrize("env,dtype,K", [({"RM_DEBUG_HBM_LISTS": "1"}, F32, 10), ({"RM_DEBUG_HBM_LISTS": "1"}, F64, 10),
                                          ({"RM_DEBUG_LANE_CAP_MIN": "1"}, F32, 100), ({"RM_DEBUG_LANE_CAP_MIN": "1"}, F64, 50),
                                          ({"RM_DEBUG_LANE_MIN_K": "1000000"}, F64, 12), ({"RM_DEBUG_SPLITS": "3,2,5"}, F32, 10),
                                          ({"RM_DEBUG_NO_TRAIN_BITS": "1"}, F32, 10), ({"RM_DEBUG_NO_TRAIN_BITS": "1"}, F32, 100)])
def test_forced_list_schemes(hip, oracle, monkeypatch, env, dtype, K):
    """the existing switches: replace-the-minimum lists in HBM, the smallest lane buffers (a selection every few tiles), fp64 lists in
    LDS, several item ranges (more parts to merge), the CSR cursor instead of dense train rows"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    A, B, excl = iid_problem(300, 5000, 64, dtype, 1064)
    check_problem(hip, oracle, A, B, excl, K, dtype, str(env), min_coverage=0.95)


# ---- the users only this call serves --------------------------------------------------------------------------------------------
_SHORT_ENVS = [{}, {"RM_DEBUG_HBM_LISTS": "1"}, {"RM_DEBUG_LANE_CAP_MIN": "1"}, {"RM_DEBUG_SAMPLE_SEED": "64"}]


@pytest.mark.parametrize("env", _SHORT_ENVS, ids=["default", "hbm-lists", "lane-cap-min", "sample-64"])
@pytest.mark.parametrize("K", [10, 100, 300, 1500])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_users_with_few_candidates(hip, oracle, monkeypatch, dtype, K, env):
    """planted into one problem: an empty row, the whole catalogue (status 1), and C = 1, 3, K - 1, K, K + 1 candidates -- at a K of
    every list scheme (LDS / HBM lists, lane buffers + k_collect_topk of two sizes, score rows + k_select_topk).  The metric call never
    activates a user with fewer candidates than K: no scheme had been finalised for lists that cannot fill."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    m, n = 80, 2000
    A, B, excl = iid_problem(m, n, 64, dtype, 31)
    rows = {0: n, 3: 0, 5: 1, 6: 3, 40: K - 1, 41: K, 42: K + 1, 77: 1, 78: 3, 79: K - 1}
    excl = plant_rows(excl, n, rows)
    got = check_problem(hip, oracle, A, B, excl, K, dtype, "few candidates K=%d" % K)
    ids, sc, st = got
    assert st[3] == 1 and (ids[3] == -1).all() and np.isnan(sc[3]).all()
    for u, c in rows.items():
        if c:
            assert st[u] == 0 and (ids[u, :min(c, K)] >= 0).all() and (ids[u, min(c, K):] == -1).all() and np.isnan(sc[u, min(c, K):]).all()


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("K", [10, 100])
def test_no_exclusion_matrix_at_all(hip, oracle, dtype, K):
    A, B, _ = iid_problem(300, 5000, 50, dtype, 1050)
    got = run_host(hip, A, B, None, K)
    S = oracle.scores(A, B, dtype=dtype)
    check_lists(got, expected_lists(S, None, K), "no exclusion matrix")
    empty = (np.zeros(A.shape[0] + 1, np.int32), np.zeros(0, np.int32))
    cross_check_with_oracle_rank(oracle, A, B, empty, K, got, dtype, 0.95, "no exclusion matrix")
    check_lists(run_host(hip, A, B, empty, K), got, "an empty matrix is no matrix")


# ---- exact ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 16), (F32, 100), (F64, 16)])
def test_exact_ties_inside_the_list_and_across_its_edge(hip, oracle, dtype, K):
    A, B, excl = iid_problem(257, 5000, 12, dtype, 99, quarters=True)
    S = oracle.scores(A, B, dtype=dtype)
    want = expected_lists(S, excl, K)
    inside = sum(1 for u in range(A.shape[0]) if want[2][u] == 0 and (np.diff(want[1][u][~np.isnan(want[1][u])]) == 0).any())
    assert inside > A.shape[0] // 2, "the inputs do not tie: %d users" % inside
    got = run_host(hip, A, B, excl, K)
    check_lists(got, want, "quarters")
    cross_check_with_oracle_rank(oracle, A, B, excl, K, got, dtype, 0.95, "quarters")


@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 100), (F32, 300), (F64, 10)])
def test_all_scores_equal(hip, oracle, dtype, K):
    """B constant: every candidate ties -- the list is the K smallest candidate ids (the metric call calls such a user invalid)"""
    A, B, excl = iid_problem(120, 3000, 16, dtype, 5)
    B = np.full_like(B, 0.25)
    got = check_problem(hip, oracle, A, B, excl, K, dtype, "all equal", cross=False)
    p, i = excl
    for u in (0, 7, 119):
        keep = np.ones(B.shape[0], bool)
        keep[i[p[u]:p[u + 1]]] = False
        assert got[0][u].tolist() == np.flatnonzero(keep)[:K].tolist()


# ---- ordered / structured scores at C2's item count ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("kind,dtype,kf", [("ascending", F32, 40), ("descending", F32, 40), ("runs", F32, 40), ("ascending", F32, 1),
                                           ("ascending", F64, 24), ("descending", F64, 24), ("runs", F64, 24)])
def test_structured_scores(hip, oracle, kind, dtype, kf, K):
    """the order-adversarial inputs of tests/test_hip_structured.py: scores that ascend / descend along the item axis, runs of ties"""
    from recometrics_amd.synth import make_structured
    pr = make_structured(kind, 150, 26744, kf, dtype, mean_c=260, seed=3 + kf)
    n = pr["B"].shape[0]
    excl = plant_rows(pr["train"], n, {2: n, 3: 0, 4: 3})
    check_problem(hip, oracle, pr["A"], pr["B"], excl, K, dtype, kind, min_coverage=0.95 if kind != "runs" else None)


# ---- non-finite scores --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 100), (F64, 10), (F32, 300)])
@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_non_finite_item_row(hip, oracle, dtype, K, poison):
    """one item's factors hold a NaN / +Inf: status 2 for every user that does not exclude the item, correct lists for the others"""
    A, B, excl = iid_problem(300, 5000, 64, dtype, 1064)
    B = B.copy()
    item = 1234
    B[item, 5] = poison
    p, i = excl
    if item not in i[p[11]:p[12]]:                        # somebody with an ordinary row excludes the item
        row = np.sort(np.concatenate([i[p[11]:p[12]], np.array([item], np.int32)]))
        i = np.concatenate([i[:p[11]], row, i[p[12]:]]).astype(np.int32)
        p = p.copy()
        p[12:] += 1
        excl = (p, i)
    excludes = np.array([item in i[p[u]:p[u + 1]] for u in range(A.shape[0])])
    got = check_problem(hip, oracle, A, B, excl, K, dtype, "poison %r" % poison, cross=False)
    st = got[2]
    C = B.shape[0] - np.diff(p)
    assert excludes[11] and (st[(C > 0) & ~excludes] == 2).all() and (st[(C > 0) & excludes] == 0).all()


# ---- CSR validation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F64, 100)])
def test_unsorted_rows_and_bad_indices(hip, oracle, dtype, K):
    A, B, excl = iid_problem(300, 5000, 64, dtype, 1064)
    p, i = excl
    rng = np.random.default_rng(3)
    shuffled = i.copy()
    for u in range(0, A.shape[0], 3):
        shuffled[p[u]:p[u + 1]] = rng.permutation(shuffled[p[u]:p[u + 1]])
    assert (shuffled != i).any()
    keep = shuffled.copy()
    check_lists(run_host(hip, A, B, (p, shuffled), K), run_host(hip, A, B, excl, K), "unsorted rows")
    assert (shuffled == keep).all(), "the caller's arrays were modified"
    bad = i.copy()
    bad[p[17]] = B.shape[0]
    with pytest.raises(ValueError, match="row 17"):
        run_host(hip, A, B, (p, bad), K)
    badp = p.copy()
    badp[30] = p[31] + 5
    with pytest.raises(ValueError, match="row"):
        run_host(hip, A, B, (badp, i), K)
    check_lists(run_host(hip, A, B, excl, K), expected_lists(oracle.scores(A, B, dtype=dtype), excl, K), "after the errors")


# ---- consistency with rm_rank_* -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 100), (F32, 300), (F64, 10), (F64, 100)])
def test_agrees_with_rank_on_the_users_it_ranks(hip, dtype, K):
    from recometrics_amd.synth import make_problem
    pr = make_problem(400, 6000, 64, dtype, mean_c=50, seed=21)
    trp, tri = pr["train"]
    tep, tei, _ = pr["test"]
    rk = hip.rank(pr["A"], pr["B"], trp, tri, tep, tei, K, break_ties_with_noise=False)
    ids, sc, st = run_host(hip, pr["A"], pr["B"], (trp, tri), K)
    ranked = np.flatnonzero(rk["status"] == 0)
    assert ranked.shape[0] > 350
    assert (st[ranked] == 0).all() and (ids[ranked] == rk["topk_idx"][ranked]).all()
    assert_same_bits(sc[ranked], rk["topk_score"][ranked], "scores against rm_rank")


# ---- the device entry ---------------------------------------------------------------------------------------------------------------
_DEVICE_ENTRY_SCRIPT = r"""
import json, os, sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch                                           # (before the library: the order bench.py loads them in)
from recometrics_amd import _binding as hip
from test_hip_recommend import check_lists, iid_problem, run_host
torch.cuda.set_device(0); hip.load(); hip.set_device(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
m, n, kf = 300, 5000, 64
done = []
for dtype, K in ((np.float32, 10), (np.float32, 100), (np.float32, 300), (np.float32, 1500), (np.float64, 10), (np.float64, 100)):
    A, B, excl = iid_problem(m, n, kf, dtype, 1064)
    want = run_host(hip, A, B, excl, K)
    tA, tB = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    tp, ti = torch.from_numpy(excl[0]).to(dev), torch.from_numpy(excl[1]).to(dev)
    idx = torch.full((m, K), 77, dtype=torch.int32, device=dev)
    sc = torch.full((m, K), 7.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=dev)
    st = torch.full((m,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    args = (dtype, tA.data_ptr(), kf, tB.data_ptr(), kf, m, n, kf, tp.data_ptr(), ti.data_ptr(), int(ti.shape[0]), K)
    hip.recommend_device(*args, idx.data_ptr(), sc.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    check_lists((idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), want, "device entry")
    tm = hip.timings()
    assert tm["device_ms"] > 0 and tm["sweep_ms"] > 0 and tm["finalize_ms"] > 0, tm
    # score = NULL: ids only, the score tensor is left alone
    idx.fill_(77); st.fill_(77); sc.fill_(7.0)
    torch.cuda.synchronize()
    hip.recommend_device(*args, idx.data_ptr(), 0, st.data_ptr(), stream)
    torch.cuda.synchronize()
    check_lists((idx.cpu().numpy(), None, st.cpu().numpy()), want, "device entry, ids only")
    assert bool((sc == 7.0).all())
    # no exclusion matrix
    hip.recommend_device(dtype, tA.data_ptr(), kf, tB.data_ptr(), kf, m, n, kf, 0, 0, 0, K, idx.data_ptr(), sc.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    check_lists((idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), run_host(hip, A, B, None, K), "device entry, nothing excluded")
    done.append([np.dtype(dtype).name, K])
print(json.dumps(done))
"""


def test_device_entry(hip):
    """torch device tensors in, lists in device tensors out, equal to the host entry's (itself checked against the oracle above), at a
    K of every list scheme; score = NULL; no exclusion matrix; rm_get_timings.  (A process of its own: the tensors are torch's, and
    torch wants to be loaded before the library.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _DEVICE_ENTRY_SCRIPT % {"root": root}], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert len(json.loads(res.stdout.strip().splitlines()[-1])) == 6


@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 100), (F64, 10)])
def test_host_entry_ids_only(hip, dtype, K):
    A, B, excl = iid_problem(300, 5000, 64, dtype, 1064)
    ids_only = run_host(hip, A, B, excl, K, scores=False)
    assert ids_only[1] is None
    check_lists(ids_only, run_host(hip, A, B, excl, K), "host entry, ids only")


# ---- results depend neither on the device list nor on the batch size ---------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 100), (F32, 300), (F64, 10)])
def test_shards_and_batches_change_nothing(hip, monkeypatch, dtype, K):
    from recometrics_amd.synth import make_factors, make_interactions_fast
    m, n, kf = 5000, 3000, 32
    A, B = make_factors(m, n, kf, dtype, 4)
    trp, tri = make_interactions_fast(m, n, 40, dtype, 4)[:2]
    excl = plant_rows((trp, tri), n, {0: 0, 1023: 0, 1024: 3, 2048: n, m - 1: 1})
    plain = run_host(hip, A, B, excl, K)
    assert (plain[2] == 0).sum() == m - 2 and (plain[2] == 1).sum() == 2
    hip.set_devices([0, 0, 0])
    try:
        check_lists(run_host(hip, A, B, excl, K), plain, "three shards")
    finally:
        hip.set_devices([])
    monkeypatch.setenv("RM_BATCH_USERS", "1024")
    check_lists(run_host(hip, A, B, excl, K), plain, "batches of 1,024 users")
    hip.set_devices([0, 0])
    try:
        check_lists(run_host(hip, A, B, excl, K), plain, "two shards in batches")
    finally:
        hip.set_devices([])


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_recommend_topk(hip, oracle, dtype):
    from scipy.sparse import coo_array, csr_array
    from recometrics_amd import recommend_topk
    m, n, kf, K = 300, 5000, 50, 10
    A, B, excl = iid_problem(m, n, kf, dtype, 1050)
    X = csr_array((np.ones(excl[1].shape[0], dtype), excl[1], excl[0]), shape=(m, n))
    S = oracle.scores(A, B, dtype=dtype)
    want = expected_lists(S, excl, K)
    check_lists(recommend_topk(A, B, k=K, X_train=X), want, "csr")
    # int64 index arrays, another format, the caller's matrix untouched
    X64 = csr_array((X.data, X.indices.astype(np.int64), X.indptr.astype(np.int64)), shape=X.shape)
    check_lists(recommend_topk(A, B, k=K, X_train=X64), want, "int64 indices")
    assert X64.indices.dtype == np.int64 and X64.indptr.dtype == np.int64
    check_lists(recommend_topk(A, B, k=K, X_train=coo_array(X)), want, "coo")
    # a subset of the users in a permuted order
    users = np.random.default_rng(1).permutation(m)[:97]
    users[:3] = [1, m // 2, m - 2]                      # the planted rows: empty, full, all but three
    got = recommend_topk(A, B, k=K, X_train=X, users=users)
    check_lists(got, tuple(w[users] for w in want), "users=")
    # ids only
    ids, sc, st = recommend_topk(A, B, k=K, X_train=X, return_scores=False)
    assert sc is None
    check_lists((ids, None, st), want, "ids only")
    # strided A (a row-major view with a leading dimension of its own)
    wide = np.zeros((m, kf + 7), dtype)
    wide[:, :kf] = A
    check_lists(recommend_topk(wide[:, :kf], B, k=K, X_train=X), want, "strided A")
    # item biases next to the factors: one more factor
    bias = np.random.default_rng(2).standard_normal(n).astype(dtype)
    Ab, Bb = np.hstack([A, np.ones((m, 1), dtype)]), np.hstack([B, bias.reshape(-1, 1)])
    check_lists(recommend_topk(A, B, k=K, X_train=X, item_biases=bias), expected_lists(oracle.scores(Ab, Bb, dtype=dtype), excl, K), "item biases")
    # the non-personalised ranking (float64, as in calc_reco_metrics)
    Sb = oracle.scores(np.ones((m, 1)), bias.astype(np.float64).reshape(-1, 1), dtype=F64)
    check_lists(recommend_topk(None, None, k=K, X_train=X, item_biases=bias), expected_lists(Sb, excl, K), "biases alone")
    # mixed precision -> float64
    got = recommend_topk(A.astype(F64), B.astype(F32), k=K, X_train=X)
    assert got[1].dtype == F64
    check_lists(got, expected_lists(oracle.scores(A.astype(F64), B.astype(F32).astype(F64), dtype=F64), excl, K), "mixed precision")
    # no exclusion matrix
    check_lists(recommend_topk(A, B, k=K), expected_lists(S, None, K), "X_train=None")


# ---- one full-size case ---------------------------------------------------------------------------------------------------------------
def stratified_sample(excl_p, m, count, seed=0):
    """first / last user block, the heaviest and the emptiest rows, random rest"""
    ln = np.diff(excl_p)
    order = np.argsort(ln, kind="stable")
    pick = set(range(128)) | set(range(m - 128, m)) | set(order[:128].tolist()) | set(order[-128:].tolist())
    rng = np.random.default_rng(seed)
    for u in rng.permutation(m):
        if len(pick) >= count:
            break
        pick.add(int(u))
    return np.array(sorted(pick), np.int64)


def test_c2_shape_full_user_count(hip, oracle):
    """BASELINE C2's shape (138,493 users x 26,744 items x 64 factors, K = 10), every user through the call, checker (1) on a
    stratified sample of 2,048 users: the oracle's scores for the full matrix (3.7 G entries, a serial fma chain each) are too slow to
    be worth it -- the sample holds the first and the last user block, the 128 heaviest and the 128 emptiest rows and a random rest."""
    from recometrics_amd.synth import CONFIGS, make_factors, make_interactions_fast
    m, n, kf, dtype, K, mean_c, seed = CONFIGS["C2"]
    A, B = make_factors(m, n, kf, dtype, seed)
    trp, tri = make_interactions_fast(m, n, mean_c, dtype, seed)[:2]
    excl = plant_rows((trp, tri), n, {5: n, 6: 0, 7: 3, m - 3: 0, m - 2: K - 1})
    ids, sc, st = run_host(hip, A, B, excl, K)
    assert (st == 1).sum() == 2 and (st == 0).sum() == m - 2
    users = stratified_sample(excl[0], m, 2048)
    assert users.shape[0] == 2048 and {5, 6, 7, m - 3, m - 2} <= set(users.tolist())
    S = oracle.scores(A[users], B, dtype=dtype)
    check_lists((ids[users], sc[users], st[users]), expected_lists(S, excl, K, users), "C2 sample")
    # every row is well-formed, sample or not: ids in range and distinct, scores descending
    full = np.flatnonzero((st == 0) & (n - np.diff(excl[0]) >= K))
    assert full.shape[0] >= m - 5 and ((ids[full] >= 0) & (ids[full] < n)).all()
    srt = np.sort(ids[full], axis=1)
    assert (np.diff(sc[full], axis=1) <= 0).all() and (srt[:, 1:] != srt[:, :-1]).all()
