"""GPU: the recommendation lists from a caller's score matrix (rm_recommend_scores_* / recommend_topk_from_scores).

The expected values need no oracle: for a given S they are `expected_lists` of tests/test_hip_recommend.py (numpy lexsort on the
candidates: score descending, item id ascending; status 1 for an empty candidate set, 2 when a candidate score is not finite) applied
to S with -0 replaced by +0.  No sampling and no tolerance: every user, ids equal, scores equal in every bit, status equal.

The row kernel (k_topk_rows, csrc/rm_rowtopk.hpp) serves k_top <= 1024: an append buffer of CAP = 2048 pairs in LDS, compacted by a
bitonic network in front of a step that could overflow it (a step = 256 threads x one 16-byte load: 1,024 fp32 / 512 fp64 scores) and
as soon as it holds max(4 k_top, 256) pairs.
Beyond 1024, and under RM_DEBUG_NO_ROW_TOPK=1, the stored-row path (k_score_rows -> k_select_topk -> k_finalize_reco)."""
import functools

import numpy as np
import pytest

from test_hip_recommend import check_lists, expected_lists, iid_problem, plant_rows

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ROW_TOPK_MAX_K, CAP = 1024, 2048                      # csrc/rm_rowtopk.hpp
PASS = {F32: 1024, F64: 512}                          # scores of one step of the row walk: 256 threads x 16 bytes


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


def canonical(S):
    """-0 -> +0 (the contract: the two zeros are equal scores and come out as +0)"""
    return np.where(S == 0, np.zeros((), S.dtype), S)


def run_host(hip, S, excl, K, scores=True):
    lds = S.strides[0] // S.itemsize
    return hip.recommend_scores(S, lds, None if excl is None else excl[0], None if excl is None else excl[1], K, scores)


def check_scores(hip, S, excl, K, what):
    got = run_host(hip, S, excl, K)
    check_lists(got, expected_lists(canonical(np.ascontiguousarray(S)), excl, K), what)
    return got


def random_excl(m, n, density, seed, empty=(), full=()):
    """sorted exclusion rows: every item with probability `density`; the rows of `empty` exclude nothing, those of `full` everything"""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(m):
        if u in full:
            rows.append(np.arange(n, dtype=np.int32))
        elif u in empty:
            rows.append(np.zeros(0, np.int32))
        else:
            rows.append(np.flatnonzero(rng.random(n) < density).astype(np.int32))
    p = np.zeros(m + 1, np.int64)
    np.cumsum([r.shape[0] for r in rows], out=p[1:])
    return p.astype(np.int32), np.concatenate(rows).astype(np.int32)


def strided_view(m, n, lds, off, dtype, seed):
    """[m, n] scores whose first element sits `off` elements past a 16-byte boundary, rows `lds` elements apart"""
    raw = np.zeros(m * lds + off + 16, dtype)
    a0 = (-raw.ctypes.data % 16) // raw.itemsize                     # first 16-byte aligned element
    view = raw[a0 + off:a0 + off + m * lds].reshape(m, lds)[:, :n]
    assert (view.ctypes.data - off * raw.itemsize) % 16 == 0
    raw[...] = np.nan                                                # (whatever lies between the rows is never a score)
    view[...] = np.random.default_rng(seed).standard_normal((m, n)).astype(dtype)
    return view


# ---- 1. the loader's edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 257, 1027])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_loader_edges(hip, dtype, n):
    m = 37
    excl = random_excl(m, n, 0.3, n, empty=(0,), full=(1,))
    for off in (1, 2, 3):
        S = strided_view(m, n, n + 3, off, dtype, 10 * n + off)
        for K in sorted({1, min(10, n), n}):
            check_scores(hip, S, excl, K, "n=%d off=%d K=%d" % (n, off, K))


# ---- 2. two pieces of the train-item bitmap -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_two_bitmap_pieces(hip, dtype):
    m, n, K = 16, 32768 + 517, 10
    p, i = random_excl(m, n, 0.002, 5, empty=(14, 15))
    rows = [i[p[u]:p[u + 1]] for u in range(m)]
    edge = np.arange(32766, 32770, dtype=np.int32)
    for u in range(0, 8):                                           # these users exclude the items on both sides of the piece boundary
        rows[u] = np.union1d(rows[u], edge).astype(np.int32)
    for u in range(8, 14):
        rows[u] = np.setdiff1d(rows[u], edge).astype(np.int32)
    rows[15] = np.arange(32768 + 3, n, 7, dtype=np.int32)           # only items of the second piece
    q = np.zeros(m + 1, np.int64)
    np.cumsum([r.shape[0] for r in rows], out=q[1:])
    excl = (q.astype(np.int32), np.concatenate(rows).astype(np.int32))
    S = np.random.default_rng(6).standard_normal((m, n)).astype(dtype)
    S[:, 32760:32776] += 20                                         # the boundary's items would lead every list
    S[15, 32768:] += 20
    got = check_scores(hip, S, excl, K, "two pieces")
    assert not np.isin(got[0][:8], edge).any() and not np.isin(got[0][15], rows[15]).any()
    assert (got[0][8:14] >= 32760).all() and (got[0][8:14] < 32776).all() and (got[0][15] >= 32760).all()


# ---- 3. every k_top boundary --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def boundary_problem(dtype):
    m, n = 48, 6000
    S = np.random.default_rng(33).standard_normal((m, n)).astype(dtype)
    excl = random_excl(m, n, 0.01, 34, empty=(3,), full=(5,))
    return S, excl


@pytest.mark.parametrize("K", [1, 10, 255, 256, 257, 1023, 1024])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_k_top_on_the_fused_path(hip, dtype, K):
    S, excl = boundary_problem(dtype)
    check_scores(hip, S, excl, K, "fused K=%d" % K)
    assert hip.timings()["sweep_blocks"] == S.shape[0]              # a block per user of the call: the row kernel ran


@pytest.mark.parametrize("K", [1025, 3000])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_k_top_on_the_stored_row_path(hip, dtype, K):
    S, excl = boundary_problem(dtype)
    check_scores(hip, S, excl, K, "stored rows K=%d" % K)


@pytest.mark.parametrize("K", [10, 1024])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_both_paths_agree(hip, monkeypatch, dtype, K):
    S, excl = boundary_problem(dtype)
    fused = run_host(hip, S, excl, K)
    monkeypatch.setenv("RM_DEBUG_NO_ROW_TOPK", "1")
    hip.reload_switches()
    stored = run_host(hip, S, excl, K)
    monkeypatch.delenv("RM_DEBUG_NO_ROW_TOPK")
    hip.reload_switches()
    check_lists(stored, fused, "RM_DEBUG_NO_ROW_TOPK=1")
    check_lists(fused, expected_lists(canonical(S), excl, K), "default")


# ---- 4. users with few candidates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 1024])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_users_with_few_candidates(hip, dtype, K):
    m, n = 80, 2000
    S = np.random.default_rng(41).standard_normal((m, n)).astype(dtype)
    excl = random_excl(m, n, 0.02, 42)
    rows = {0: n, 3: 0, 5: 1, 6: 3, 40: K - 1, 41: K, 42: K + 1, 77: 1, 78: 3, 79: K - 1}      # user: number of candidates
    excl = plant_rows(excl, n, rows)
    ids, sc, st = check_scores(hip, S, excl, K, "few candidates K=%d" % K)
    assert st[3] == 1 and (ids[3] == -1).all() and np.isnan(sc[3]).all()
    for u, c in rows.items():
        if c:
            assert st[u] == 0 and (ids[u, :min(c, K)] >= 0).all() and (ids[u, min(c, K):] == -1).all() and np.isnan(sc[u, min(c, K):]).all()


# ---- 5. compaction under the worst order --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 1024])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_compaction_under_the_worst_order(hip, dtype, K):
    m, n = 24, 20000
    item = np.arange(n, dtype=np.float64)
    S = np.empty((m, n), dtype)
    for u in range(m):
        if u % 3 == 0:
            S[u] = item * 0.5 + u                                   # strictly ascending in item id: every candidate beats the bound
        elif u % 3 == 1:
            S[u] = -item * 0.5 - u                                  # strictly descending
        else:
            S[u] = np.floor(item / 64) * (1 if u % 2 else -1)       # runs of 64 equal scores, ascending / descending
    assert (np.diff(S[0]) > 0).all() and (np.diff(S[1]) < 0).all()
    excl = random_excl(m, n, 0.002, 51, empty=(0,))
    # An ascending row appends every one of its C candidates.  The buffer holds CAP pairs, a compaction keeps K of them and comes at
    # the latest when fewer than a step's PASS places are free: C appends need at least (C - CAP) / (CAP - K) compactions.
    C = n - np.diff(excl[0]).max()
    assert K + PASS[dtype] <= CAP and -(-(C - CAP) // (CAP - K)) >= 3
    check_scores(hip, S, excl, K, "worst order K=%d" % K)


# ---- 6. ties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 16), (F32, 100), (F64, 16)])
def test_exact_ties_inside_the_list_and_across_its_edge(hip, dtype, K):
    m, n = 129, 3000
    S = (np.round(np.random.default_rng(61).standard_normal((m, n)) * 4) / 4).astype(dtype)
    excl = random_excl(m, n, 0.01, 62)
    want = expected_lists(canonical(S), excl, K)
    inside = sum(1 for u in range(m) if want[2][u] == 0 and (np.diff(want[1][u][~np.isnan(want[1][u])]) == 0).any())
    assert inside > m // 2, "the inputs do not tie: %d users" % inside
    check_lists(run_host(hip, S, excl, K), want, "quarters")


@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 300), (F64, 10), (F64, 1024)])
def test_all_scores_equal(hip, dtype, K):
    m, n = 40, 3000
    S = np.full((m, n), 0.25, dtype)
    excl = random_excl(m, n, 0.05, 63, empty=(7,))
    got = check_scores(hip, S, excl, K, "all equal")
    p, i = excl
    for u in (0, 7, m - 1):
        assert got[0][u].tolist() == np.setdiff1d(np.arange(n), i[p[u]:p[u + 1]])[:K].tolist()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_two_zeros_are_one_score(hip, dtype):
    m, n, K = 20, 2500, 40
    rng = np.random.default_rng(64)
    S = np.where(rng.random((m, n)) < 0.5, 0.0, -0.0).astype(dtype)
    S[m // 2:] = np.where(rng.random((m - m // 2, n)) < 0.9, S[m // 2:], -1.0)        # (zeros lead these rows, negative scores follow)
    S[1] = -0.0
    assert np.signbit(S).any() and (~np.signbit(S)).any()
    excl = random_excl(m, n, 0.01, 65, empty=(0,))
    ids, sc, st = check_scores(hip, S, excl, K, "zeros")
    assert (st == 0).all() and (sc == 0).all() and not np.signbit(sc).any()
    p, i = excl
    for u in (0, 1, 5):                                              # all zeros: the K smallest candidate ids
        assert ids[u].tolist() == np.setdiff1d(np.arange(n), i[p[u]:p[u + 1]])[:K].tolist()


# ---- 7. non-finite scores -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 1025])
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_non_finite_scores(hip, dtype, poison, K):
    m, n = 40, 3000
    S0 = np.random.default_rng(71).standard_normal((m, n)).astype(dtype)
    excl = random_excl(m, n, 0.02, 72)
    clean = check_scores(hip, S0, excl, K, "clean")
    p, i = excl
    S = S0.copy()
    for u in (4, 11):                                               # at an item the user excludes: never looked at
        S[u, i[p[u] + 2]] = poison
    hit = {}
    for u in (9, 30):                                               # at a candidate (the first and some later one)
        cand = np.setdiff1d(np.arange(n), i[p[u]:p[u + 1]])
        hit[u] = cand[0] if u == 9 else cand[cand.shape[0] // 2]
        S[u, hit[u]] = poison
    ids, sc, st = check_scores(hip, S, excl, K, "poison %r" % poison)
    others = np.setdiff1d(np.arange(m), list(hit))
    assert (st[others] == 0).all() and (st[list(hit)] == 2).all()
    assert (ids[list(hit)] == -1).all() and np.isnan(sc[list(hit)]).all()
    check_lists((ids[others], sc[others], st[others]), tuple(c[others] for c in clean), "the other users")


# ---- 8. the same bits as the factor call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 100, 300])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_same_bits_as_the_factor_call(hip, oracle, dtype, K):
    A, B, excl = iid_problem(300, 5000, 64, dtype, 1064)
    S = oracle.scores(A, B, dtype=dtype)
    want = hip.recommend(A, A.shape[1], B, B.shape[1], excl[0], excl[1], K)
    check_lists(run_host(hip, S, excl, K), want, "against rm_recommend")


# ---- 9. CSR handling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F64, 100), (F32, 1025)])
def test_unsorted_rows_and_bad_indices(hip, dtype, K):
    m, n = 300, 5000
    S = np.random.default_rng(91).standard_normal((m, n)).astype(dtype)
    p, i = random_excl(m, n, 0.01, 92)
    rng = np.random.default_rng(3)
    shuffled = i.copy()
    for u in range(0, m, 3):
        shuffled[p[u]:p[u + 1]] = rng.permutation(shuffled[p[u]:p[u + 1]])
    assert (shuffled != i).any()
    keep = shuffled.copy()
    want = expected_lists(canonical(S), (p, i), K)
    check_lists(run_host(hip, S, (p, shuffled), K), want, "unsorted rows")
    assert (shuffled == keep).all(), "the caller's arrays were modified"
    bad = i.copy()
    bad[p[17]] = n
    with pytest.raises(ValueError, match="row 17"):
        run_host(hip, S, (p, bad), K)
    badp = p.copy()
    badp[30] = p[31] + 5
    with pytest.raises(ValueError, match="row"):
        run_host(hip, S, (badp, i), K)
    check_lists(run_host(hip, S, (p, i), K), want, "after the errors")


# ---- 10. results depend neither on the device list nor on the batch size ------------------------------------------------------------
@pytest.mark.parametrize("dtype,K", [(F32, 10), (F32, 300), (F64, 10)])
def test_shards_and_batches_change_nothing(hip, monkeypatch, dtype, K):
    from recometrics_amd.synth import make_interactions_fast
    m, n = 5000, 700
    S = np.random.default_rng(101).standard_normal((m, n)).astype(dtype)
    trp, tri = make_interactions_fast(m, n, 20, dtype, 4)[:2]
    excl = plant_rows((trp, tri), n, {0: 0, 1023: 0, 1024: 3, 2048: n, m - 1: 1})
    plain = run_host(hip, S, excl, K)
    assert (plain[2] == 0).sum() == m - 2 and (plain[2] == 1).sum() == 2
    users = np.r_[0:40, 1000:1050, 2040:2060, m - 30:m]
    check_lists(tuple(x[users] for x in plain), expected_lists(S[users], excl, K, users), "unsharded, a sample against numpy")
    hip.set_devices([0, 0, 0])
    try:
        check_lists(run_host(hip, S, excl, K), plain, "three shards")
    finally:
        hip.set_devices([])
    monkeypatch.setenv("RM_BATCH_USERS", "1024")
    check_lists(run_host(hip, S, excl, K), plain, "batches of 1,024 users")
    hip.set_devices([0, 0, 0])
    try:
        check_lists(run_host(hip, S, excl, K), plain, "three shards in batches")
    finally:
        hip.set_devices([])


# ---- 11. the device entry -------------------------------------------------------------------------------------------------------------
_DEVICE_ENTRY_SCRIPT = r"""
import json, os, sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch                                           # (before the library: the order bench.py loads them in)
from recometrics_amd import _binding as hip
from test_hip_recommend import check_lists, expected_lists
from test_hip_recommend_scores import canonical, random_excl
torch.cuda.set_device(0); hip.load(); hip.set_device(0)
dev = torch.device("cuda", 0)
side = torch.cuda.Stream(device=dev)
m, n = 300, 5000
ld = n + 3
excl = random_excl(m, n, 0.01, 111, empty=(2,), full=(7,))
tp, ti = torch.from_numpy(excl[0]).to(dev), torch.from_numpy(excl[1]).to(dev)
done = []


def call(dtype, view, K, idx, sc, st, with_excl=True):
    hip.recommend_scores_device(dtype, view.data_ptr(), ld, m, n, tp.data_ptr() if with_excl else 0, ti.data_ptr() if with_excl else 0,
                                int(ti.shape[0]) if with_excl else 0, K, idx.data_ptr(), sc.data_ptr() if sc is not None else 0, st.data_ptr(),
                                side.cuda_stream)
    side.synchronize()


for dtype, K in ((np.float32, 10), (np.float32, 1024), (np.float32, 1025), (np.float64, 10), (np.float64, 100)):
    S = np.random.default_rng(112).standard_normal((m, n)).astype(dtype)
    wide = torch.zeros((m, ld), dtype=torch.float32 if dtype == np.float32 else torch.float64, device=dev)
    view = wide[:, :n]
    view.copy_(torch.from_numpy(S))
    want = expected_lists(canonical(S), excl, K)
    idx = torch.full((m, K), 77, dtype=torch.int32, device=dev)
    sc = torch.full((m, K), 7.0, dtype=wide.dtype, device=dev)
    st = torch.full((m,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    call(dtype, view, K, idx, sc, st)
    check_lists((idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), want, "device entry")
    tm = hip.timings()
    assert tm["device_ms"] > 0 and tm["sweep_ms"] > 0 and tm["sweep_blocks"] > 0, tm
    # score = NULL: ids only, the score tensor is left alone
    idx.fill_(77); st.fill_(77); sc.fill_(7.0)
    torch.cuda.synchronize()
    call(dtype, view, K, idx, None, st)
    check_lists((idx.cpu().numpy(), None, st.cpu().numpy()), want, "device entry, ids only")
    assert bool((sc == 7.0).all())
    # no exclusion matrix
    call(dtype, view, K, idx, sc, st, with_excl=False)
    check_lists((idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), expected_lists(canonical(S), None, K), "device entry, nothing excluded")
    done.append([np.dtype(dtype).name, K])
# a device with 8 MB: the masked rows of these users alone are 12 MB (fp64), and the row kernel keeps none of them
dtype, K = np.float64, 100
hip.load().rm_release_workspace()
os.environ["RM_DEBUG_FREE_MB"] = "8"
hip.reload_switches()
try:
    idx = torch.full((m, K), 77, dtype=torch.int32, device=dev)
    sc = torch.full((m, K), 7.0, dtype=torch.float64, device=dev)
    call(dtype, view, K, idx, sc, st)
    check_lists((idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), expected_lists(canonical(S), excl, K), "device entry, 8 MB")
    idx = torch.full((m, 1025), 77, dtype=torch.int32, device=dev)
    sc = torch.full((m, 1025), 7.0, dtype=torch.float64, device=dev)
    try:
        call(dtype, view, 1025, idx, sc, st)
        raise SystemExit("no MemoryError")
    except MemoryError as e:
        msg = str(e)
    assert "score matrix" in msg and "(%%d B) per user" %% ((n + 191) // 192 * 192 * 8) in msg and "%%d users do not fit" %% m in msg, msg
finally:
    del os.environ["RM_DEBUG_FREE_MB"]
    hip.reload_switches()
torch.cuda.synchronize()
print(json.dumps(done))
"""


def test_device_entry(hip):
    """torch device tensors in (a row stride of n + 3), lists in device tensors out on a stream that is not the default one, at a k_top
    of either path; score = NULL; no exclusion matrix; rm_get_timings; and under RM_DEBUG_FREE_MB=8 the call that keeps no score row
    succeeds where the one that stores them answers RM_ERR_NOMEM.  (A process of its own: the tensors are torch's, and torch wants to be
    loaded before the library.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _DEVICE_ENTRY_SCRIPT % {"root": root}], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert len(json.loads(res.stdout.strip().splitlines()[-1])) == 5


# ---- 12. the Python surface -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_recommend_topk_from_scores(hip, dtype):
    from scipy.sparse import coo_array, csr_array
    from recometrics_amd import recommend_topk_from_scores
    m, n, K = 300, 5000, 10
    S = np.random.default_rng(121).standard_normal((m, n)).astype(dtype)
    excl = plant_rows(random_excl(m, n, 0.01, 122), n, {1: n, m // 2: 0, m - 2: 3})
    X = csr_array((np.ones(excl[1].shape[0], dtype), excl[1], excl[0]), shape=(m, n))
    want = expected_lists(S, excl, K)
    check_lists(recommend_topk_from_scores(S, k=K, X_train=X), want, "csr")
    X64 = csr_array((X.data, X.indices.astype(np.int64), X.indptr.astype(np.int64)), shape=X.shape)
    check_lists(recommend_topk_from_scores(S, k=K, X_train=X64), want, "int64 indices")
    assert X64.indices.dtype == np.int64 and X64.indptr.dtype == np.int64
    check_lists(recommend_topk_from_scores(S, k=K, X_train=coo_array(X)), want, "coo")
    users = np.random.default_rng(1).permutation(m)[:97]
    users[:3] = [1, m // 2, m - 2]                      # the planted rows: empty, full, all but three
    check_lists(recommend_topk_from_scores(S, k=K, X_train=X, users=users), tuple(w[users] for w in want), "users=")
    ids, sc, st = recommend_topk_from_scores(S, k=K, X_train=X, return_scores=False)
    assert sc is None
    check_lists((ids, None, st), want, "ids only")
    wide = np.full((m, n + 7), np.nan, dtype)
    wide[:, 2:2 + n] = S
    check_lists(recommend_topk_from_scores(wide[:, 2:2 + n], k=K, X_train=X), want, "a column slice of a wider matrix")
    Si = np.random.default_rng(123).integers(-50, 50, (m, n)).astype(np.int32)
    got = recommend_topk_from_scores(Si, k=K, X_train=X)
    assert got[1].dtype == F64
    check_lists(got, expected_lists(Si.astype(F64), excl, K), "int32 scores")
    check_lists(recommend_topk_from_scores(S, k=K), expected_lists(S, None, K), "X_train=None")
