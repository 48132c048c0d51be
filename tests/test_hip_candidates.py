"""GPU: top-K lists from candidate sets (rm_recommend_candidates_* / recommend_topk_from_candidates, k_topk_candidates) against
S = oracle.scores(A, B) and test_hip_recommend's checker on the COMPLEMENT of the candidate rows: every user, ids, status, score bits."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _layouts as lay
from _candidates import complement_of, csr_of, rows_of, spread_rows  # noqa: F401 (spread_rows: test_cuda_tensors' script imports it from here)
from test_hip_entry_fields import dev  # noqa: F401 (a fixture)
from test_hip_recommend import check_lists, expected_lists, hip  # noqa: F401 (hip: a fixture)

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
# the step's edges (64 per wavefront, 256 per block), the append-everything limit (2,048), the first and the second compaction
EDGE_C = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2048 + 256 + 1, 4999)


@functools.lru_cache(maxsize=None)
def problem(m, n, kf, dtype):
    from recometrics_amd.synth import make_factors
    return make_factors(m, n, kf, dtype, 7)


@functools.lru_cache(maxsize=None)
def want_of(m, n, kf, dtype, counts, seed, K):
    """(candidate rows, expected lists) of problem(m, n, kf, dtype)"""
    from oracle.oracle import Oracle
    cand = spread_rows(counts, n, seed)
    return cand, expected_lists(Oracle().scores(*problem(m, n, kf, dtype), dtype=dtype), complement_of(cand, n), K)


def run_host(hip, A, B, cand, K, scores=True):
    return hip.recommend_candidates(A, A.shape[1], B, B.shape[1], cand[0], cand[1], K, scores)


def run_dev(hip, dev, A, B, cand, K, scores=True, layout="D", layout_b=None):
    """the device entry; `layout` for A and, unless `layout_b` names another, for B: a name of tests/_layouts.py or a (pad, off) pair
    in elements; NaN in every element that is not a factor"""
    dtype, m, at = A.dtype.type, A.shape[0], []
    for X, name in ((A, layout), (B, layout if layout_b is None else layout_b)):
        poison = lay.NAN_POISON[lay.PREC[np.dtype(dtype)]]
        V, raw, off = lay.place_as(X, name, poison) if isinstance(name, str) else lay.place(X, *name, poison)
        at += [dev.put(raw) + off * raw.itemsize, V.strides[0] // raw.itemsize]
    idx, sc, st = dev.put(np.full((m, K), 77, np.int32)), dev.put(np.full((m, K), 7, dtype)), dev.put(np.full(m, 77, np.int32))
    hip.recommend_candidates_device(dtype, *at, m, B.shape[0], A.shape[1], dev.put(cand[0]), dev.put(cand[1]), int(cand[1].shape[0]), K,
                                    idx, sc if scores else 0, st)
    return dev.get(idx, (m, K), np.int32), dev.get(sc, (m, K), dtype), dev.get(st, (m,), np.int32)


@pytest.mark.parametrize("K", [1, 10, 1024])
@DTYPES
def test_row_length_edges(hip, dtype, K):
    m, n, kf = 40, 5000, 24
    cand, want = want_of(m, n, kf, dtype, EDGE_C + tuple(range(100, 100 + 7 * (m - len(EDGE_C)), 7)), 1, K)
    assert np.diff(cand[0])[:len(EDGE_C)].tolist() == list(EDGE_C) and cand[1].min() == 0 and cand[1].max() == n - 1
    assert want[2][0] == 1 and (want[2][1:] == 0).all()
    check_lists(run_host(hip, *problem(m, n, kf, dtype), cand, K), want, "K = %d" % K)


@pytest.mark.parametrize("kf", [1, 3, 15, 16, 17, 64, 130])
@DTYPES
def test_factor_counts_and_layouts(hip, dev, dtype, kf):
    m, n, K = 40, 600, 10
    A, B = problem(m, n, kf, dtype)
    cand, want = want_of(m, n, kf, dtype, tuple(range(1, 1 + 8 * m, 8)), 2, K)
    dense = run_dev(hip, dev, A, B, cand, K)
    check_lists(dense, want, "dense, %d factors" % kf)
    check_lists(run_dev(hip, dev, A, B, cand, K, layout="RO"), dense, "odd stride, base one element past a 16-byte boundary")


@DTYPES
def test_ties_zeros_duplicates_order(hip, dev, dtype):
    from oracle.oracle import Oracle
    m, n, kf, K = 40, 600, 24, 50
    A, B = (x.copy() for x in problem(m, n, kf, dtype))
    B[:] = B[np.arange(n) // 5 * 5]                                   # blocks of five identical rows: equal scores, ordered by id
    A[3], A[4] = 0.0, -0.0                                            # every score +0
    clean = spread_rows(tuple(range(60, 60 + 6 * m, 6)), n, 3)
    want = expected_lists(Oracle().scores(A, B, dtype=dtype), complement_of(clean, n), K)
    got = run_host(hip, A, B, clean, K)
    check_lists(got, want, "clean rows")
    assert not np.signbit(got[1][3:5]).any() and (got[1][3:5] == 0).all() and (got[0][3] == clean[1][clean[0][3]:clean[0][3] + K]).all()
    repeated = csr_of([np.sort(np.concatenate([r, r[::3], r[:2]])) for r in rows_of(clean)])
    shuffled = csr_of([np.random.default_rng(4).permutation(r) for r in rows_of(repeated)])
    check_lists(run_host(hip, A, B, repeated, K), want, "repeated ids")
    check_lists(run_host(hip, A, B, shuffled, K), want, "repeated ids, shuffled: host entry")
    check_lists(run_dev(hip, dev, A, B, shuffled, K), want, "repeated ids, shuffled: device entry")


@DTYPES
def test_non_finite_item_rows_touch_their_users_only(hip, dtype):
    from oracle.oracle import Oracle
    m, n, kf, K = 40, 600, 24, 10
    A, finite = problem(m, n, kf, dtype)
    B = finite.copy()
    B[5], B[77, 0] = np.nan, np.inf
    rows = [np.setdiff1d(r, [5, 77]) for r in rows_of(spread_rows(tuple(range(20, 20 + 9 * m, 9)), n, 5))]
    rows[1], rows[2] = np.union1d(rows[1], [5]), np.union1d(rows[2], [77])
    cand, hit = csr_of(rows), np.isin(np.arange(m), [1, 2])
    want = expected_lists(Oracle().scores(A, finite, dtype=dtype), complement_of(cand, n), K)       # (right for everybody but users 1 and 2)
    got = run_host(hip, A, B, cand, K)
    assert (got[2] == np.where(hit, 2, 0)).all() and (got[0][hit] == -1).all() and np.isnan(got[1][hit]).all()
    check_lists(tuple(g[~hit] for g in got), tuple(w[~hit] for w in want), "users that list neither item")


@DTYPES
def test_equals_recommend_on_the_complement(hip, dtype):
    m, n, kf, K = 40, 3000, 32, 10
    A, B = problem(m, n, kf, dtype)
    cand = spread_rows((0, 1, 5, K, 300, 2500, n) + tuple(range(50, 50 + 30 * (m - 7), 30)), n, 6)
    excl = complement_of(cand, n)
    check_lists(run_host(hip, A, B, cand, K), hip.recommend(A, kf, B, kf, excl[0], excl[1], K), "rm_recommend_*")


def test_batches_shards_null_scores_guard(hip, dev, monkeypatch):
    m, n, kf, K = 3000, 500, 8, 10
    A, B = problem(m, n, kf, F32)
    cand = spread_rows(tuple(np.random.default_rng(8).integers(0, 60, m)), n, 8)
    plain = run_dev(hip, dev, A, B, cand, K)
    assert set(plain[2].tolist()) == {0, 1}
    ids_only = run_dev(hip, dev, A, B, cand, K, scores=False)
    assert (ids_only[1] == 7).all()                                   # score = NULL: the array is left alone
    check_lists((ids_only[0], None, ids_only[2]), plain, "score = NULL")
    hip.set_devices([0, 0, 0])
    try:
        check_lists(run_host(hip, A, B, cand, K), plain, "three shards")
    finally:
        hip.set_devices([])
    monkeypatch.setenv("RM_BATCH_USERS", "1024")
    check_lists(run_host(hip, A, B, cand, K), plain, "three batches")
    monkeypatch.delenv("RM_BATCH_USERS")
    assert hip.load().rm_release_workspace() == 0
    monkeypatch.setenv("RM_DEBUG_WS_GUARD", "1")
    try:
        check_lists(run_host(hip, A, B, cand, K), plain, "guarded workspace")
        damaged, checked, report = hip.ws_check()
        assert damaged == 0 and checked >= 1, report
    finally:
        monkeypatch.delenv("RM_DEBUG_WS_GUARD")
        assert hip.load().rm_release_workspace() == 0


def test_defects_of_the_candidate_rows(hip):
    m, n, kf = 40, 600, 8
    A, B = problem(m, n, kf, F32)
    cand = spread_rows((30,) * m, n, 9)
    assert [x.shape for x in hip.recommend_candidates(A[:0], kf, B, kf, cand[0][:1], cand[1], 10)] == [(0, 10), (0, 10), (0,)]
    for bad in (n, -1):
        i = cand[1].copy()
        i[cand[0][7] + 3] = bad
        with pytest.raises(ValueError, match=r"out of range \[0, 600\) in row 7"):
            run_host(hip, A, B, (cand[0], i), 10)
    p = cand[0].copy()
    p[12] = p[11] - 1
    with pytest.raises(ValueError, match=r"row 11 are negative or decreasing \(X_cand\)"):
        run_host(hip, A, B, (p, cand[1]), 10)
    with pytest.raises(RuntimeError, match="at most 1024 items"):
        run_host(hip, A, B, cand, 1025)


@DTYPES
def test_public_function(hip, dtype):
    from scipy.sparse import csr_array
    from oracle.oracle import Oracle
    from recometrics_amd import recommend_topk_from_candidates as reco
    m, n, kf, K = 40, 600, 24, 10
    A, B = problem(m, n, kf, dtype)
    cand, want = want_of(m, n, kf, dtype, tuple(range(0, 8 * m, 8)), 10, K)
    X = csr_array((np.ones(cand[1].shape[0], dtype), cand[1], cand[0]), shape=(m, n))
    users = np.array([5, 0, 39, 5, 17])
    for c in (X, cand):                                               # SciPy CSR, and the (indptr, indices) pair
        check_lists(reco(A, B, c, k=K), want, "all users")
        check_lists(reco(A, B, c, k=K, users=users), tuple(w[users] for w in want), "users=")
    bias = np.random.default_rng(2).standard_normal(n).astype(dtype)
    Sb = Oracle().scores(np.hstack([A, np.ones((m, 1), dtype)]), np.hstack([B, bias.reshape(-1, 1)]), dtype=dtype)
    check_lists(reco(A, B, X, k=K, item_biases=bias), expected_lists(Sb, complement_of(cand, n), K), "item biases")
    ids, sc, st = reco(A, B, X, k=K, return_scores=False)
    assert sc is None
    check_lists((ids, None, st), want, "ids only")


_TENSOR_SCRIPT = """
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np, torch
from recometrics_amd import recommend_topk_from_candidates as reco
from test_hip_candidates import check_lists, problem, spread_rows
A, B = problem(40, 600, 24, np.float32)
cand = spread_rows(tuple(range(0, 320, 8)), 600, 10)
want = reco(A, B, cand, k=10)
check_lists(reco(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), cand, k=10), want, "CUDA tensors")
print(int((want[2] == 0).sum()))
"""


def test_cuda_tensors_equal_the_numpy_call(hip):
    """a process of its own, as the other tensor tests: torch wants to be loaded before the library"""
    here = os.path.dirname(os.path.abspath(__file__))
    res = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT % {"root": os.path.dirname(here), "tests": here}], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert json.loads(res.stdout.strip().splitlines()[-1]) == 39
