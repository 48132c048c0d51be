"""GPU: metrics and top-K lists from a score matrix in IEEE binary16 ("f16") / bfloat16 ("bf16") -- include/recometrics_hip_half.h,
and `scores` as a torch.Tensor.

The contract is one sentence: for a 16-bit matrix S, let W be the fp32 matrix with W[u, i] == S[u, i] exactly; every entry returns what
its _f32 counterpart returns for W.  W is formed on the CPU (`widen`: NumPy's float16 -> float32, or the bf16 pattern shifted into the
upper half of an fp32) and the expected values come from code that is not under test:
  lists    `expected_lists` of tests/test_hip_recommend.py (NumPy lexsort) on canonical(W);
  metrics  oracle.calc(A = W, B = I), checker (c) of tests/test_hip_scores.py: bitwise, ROC-AUC within _util.roc_tol;
  both     the _f32 entry on W, bit for bit.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _requests import planted_problem, replace_rows
from test_hip_recommend import check_lists, expected_lists
from test_hip_recommend_scores import canonical, random_excl
from test_hip_scores import ALL, assert_all_bits, assert_like_parity, oracle_on_scores, scores_calc

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = ("f16", "bf16")
HERE = os.path.dirname(os.path.abspath(__file__))
NAN16 = 0x7fff                                        # a NaN in either format


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


# ---- the two formats on the CPU ----------------------------------------------------------------------------------------------------
def widen(bits, kind):
    """W: the fp32 value of every 16-bit pattern, exactly"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return bits.view(np.float16).astype(F32) if kind == "f16" else (bits.astype(np.uint32) << 16).view(F32)


def narrow(X, kind):
    """some 16-bit pattern near every fp32 value (f16: rounded, bf16: truncated); which one does not matter -- W is formed from the patterns"""
    X = np.ascontiguousarray(X, dtype=F32)
    return X.astype(np.float16).view(np.uint16) if kind == "f16" else (X.view(np.uint32) >> 16).astype(np.uint16)


def non_finite(bits, kind):
    return (bits & 0x7c00) == 0x7c00 if kind == "f16" else (bits & 0x7f80) == 0x7f80


def as_argument(bits, kind):
    """what the binding's 16-bit wrappers take: a float16 array, or bf16 patterns as uint16 (strides kept)"""
    return bits.view(np.float16) if kind == "f16" else bits


def strided_bits(bits, lds, off):
    """the [m, n] patterns in a buffer whose first score sits `off` elements past a 16-byte boundary, rows `lds` elements apart, NaN
    everywhere between the rows"""
    m, n = bits.shape
    raw = np.full(m * lds + off + 16, NAN16, np.uint16)
    a0 = (-raw.ctypes.data % 16) // 2
    view = raw[a0 + off:a0 + off + m * lds].reshape(m, lds)[:, :n]
    assert (view.ctypes.data - 2 * off) % 16 == 0
    view[...] = bits
    return view


def half_lists(hip, view, kind, excl, K, scores=True):
    keep = view.copy()
    got = hip.recommend_scores_half(as_argument(view, kind), view.strides[0] // 2, None if excl is None else excl[0], None if excl is None else excl[1], K, scores)
    assert (view == keep).all(), "the caller's scores were modified"
    return got


def f32_lists(hip, W, excl, K):
    return hip.recommend_scores(W, W.shape[1], None if excl is None else excl[0], None if excl is None else excl[1], K)


def check_half_lists(hip, view, kind, excl, K, what):
    """the 16-bit entry against NumPy on canonical(W) and against the _f32 entry on W"""
    W = widen(view, kind)
    got = half_lists(hip, view, kind, excl, K)
    assert got[1].dtype == F32
    check_lists(got, expected_lists(canonical(W), excl, K), "%s %s: against NumPy" % (kind, what))
    check_lists(got, f32_lists(hip, W, excl, K), "%s %s: against the _f32 entry" % (kind, what))
    return got


def half_calc(hip, view, kind, train, test, k, metrics=ALL, cumulative=False, cold=True, min_items_pool=2, min_pos_test=1):
    from oracle.oracle import NAMES
    trp, tri = [np.ascontiguousarray(x, dtype=np.int32) for x in train[:2]]
    tep, tei = [np.ascontiguousarray(x, dtype=np.int32) for x in test[:2]]
    tev = np.ascontiguousarray(test[2], dtype=F32)
    want = {name: (name in metrics) for name in hip.METRIC_ORDER}
    keep = view.copy()
    outs = hip.calc_metrics_scores_half(as_argument(view, kind), view.strides[0] // 2, trp, tri, tep, tei, tev, k, want, cumulative, cold,
                                        min_items_pool, min_pos_test, 1)
    assert (view == keep).all(), "the caller's scores were modified"
    assert all(o.dtype == F32 for o in outs)
    return {NAMES[name]: arr for name, arr in zip(hip.METRIC_ORDER, outs) if want[name]}


def csr_of(rows):
    p = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.shape[0] for r in rows], out=p[1:])
    return p.astype(np.int32), (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)


# ---- 1. every value widens exactly ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def every_pattern_problem(kind):
    n = 65536                                                           # two pieces of the train-item bitmap exactly
    rng = np.random.default_rng(1)
    bits = np.stack([rng.permutation(n).astype(np.uint16) for _ in range(4)])
    rows = [np.flatnonzero(non_finite(bits[0], kind)), np.flatnonzero(non_finite(bits[1], kind)), np.zeros(0, np.int64), np.arange(n)]
    assert rows[0].shape[0] == (2048 if kind == "f16" else 256)
    return bits, csr_of([r.astype(np.int32) for r in rows])


@pytest.mark.parametrize("K", [10, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_every_value_widens_exactly(hip, kind, K):
    """each row a permutation of all 65,536 patterns: rows 0 and 1 exclude exactly the NaN / +-Inf patterns (non-finite scores at
    excluded items are ignored), row 2 excludes nothing (status 2), row 3 everything (status 1)"""
    bits, excl = every_pattern_problem(kind)
    ids, sc, st = check_half_lists(hip, bits, kind, excl, K, "all patterns K=%d" % K)
    assert st.tolist() == [0, 0, 2, 1]
    top = np.sort(widen(np.arange(65536, dtype=np.uint16)[~non_finite(np.arange(65536, dtype=np.uint16), kind)], kind))[::-1][:K]
    assert (sc[0] == top).all() and (sc[1] == top).all()


@pytest.mark.parametrize("kind", KINDS)
def test_subnormals_are_not_flushed(hip, kind):
    """rows of nothing but subnormal patterns of both signs and zeros: the order of the list is the order of the subnormals (flushed,
    every score would be zero and the list the smallest item ids); f16 subnormals come back as fp32 normals, bf16 ones as fp32 subnormals"""
    frac = 0x3ff if kind == "f16" else 0x7f
    m, n, K = 6, 3000, 1024 if kind == "f16" else 100
    rng = np.random.default_rng(2)
    bits = (rng.integers(0, frac + 1, (m, n)) | (rng.integers(0, 2, (m, n)) << 15)).astype(np.uint16)
    assert not non_finite(bits, kind).any() and (np.abs(widen(bits, kind)) < (2.0 ** -14 if kind == "f16" else 2.0 ** -126)).all()
    ids, sc, st = check_half_lists(hip, strided_bits(bits, n + 3, 5), kind, random_excl(m, n, 0.01, 3), K, "subnormals")
    assert (st == 0).all() and (sc[:, 0] > 0).all() and (np.diff(sc, axis=1) <= 0).all() and (sc[:, 0] > sc[:, -1]).all()
    tiny = np.finfo(F32).tiny
    assert (sc[:, 0] >= tiny).all() if kind == "f16" else (sc[:, 0] < tiny).all()


# ---- 2. the loader's edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049])
@pytest.mark.parametrize("kind", KINDS)
def test_loader_edges(hip, kind, n):
    """rows `n + 3` elements apart cycle through all eight 2-byte phases of a 16-byte piece, whatever the first one's is; NaN lies between
    the rows; one row excludes nothing and one everything"""
    m = 37
    excl = random_excl(m, n, 0.3, n, empty=(0,), full=(1,))
    for off in (1, 3, 4, 7):
        bits = narrow(np.random.default_rng(10 * n + off).standard_normal((m, n)), kind)
        view = strided_bits(bits, n + 3, off)
        for K in sorted({1, min(10, n), n}):
            check_half_lists(hip, view, kind, excl, K, "n=%d off=%d K=%d" % (n, off, K))


# ---- 3. every k_top boundary ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def boundary_problem(kind):
    m, n = 48, 6000
    bits = narrow(np.random.default_rng(33).standard_normal((m, n)), kind)
    return bits, random_excl(m, n, 0.01, 34, empty=(3,), full=(5,))


@pytest.mark.parametrize("K", [1, 10, 255, 256, 257, 1023, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_k_top_on_the_row_kernel(hip, kind, K):
    bits, excl = boundary_problem(kind)
    got = half_lists(hip, bits, kind, excl, K)
    assert hip.timings()["sweep_blocks"] == bits.shape[0]               # a block per user of the call: the row kernel ran
    W = widen(bits, kind)
    check_lists(got, expected_lists(canonical(W), excl, K), "%s row kernel K=%d: against NumPy" % (kind, K))
    check_lists(got, f32_lists(hip, W, excl, K), "%s row kernel K=%d: against the _f32 entry" % (kind, K))


@pytest.mark.parametrize("K", [1025, 3000])
@pytest.mark.parametrize("kind", KINDS)
def test_k_top_on_the_stored_rows(hip, kind, K):
    bits, excl = boundary_problem(kind)
    check_half_lists(hip, bits, kind, excl, K, "stored rows K=%d" % K)


@pytest.mark.parametrize("K", [10, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_both_paths_agree(hip, monkeypatch, kind, K):
    bits, excl = boundary_problem(kind)
    fused = half_lists(hip, bits, kind, excl, K)
    monkeypatch.setenv("RM_DEBUG_NO_ROW_TOPK", "1")
    hip.reload_switches()
    stored = half_lists(hip, bits, kind, excl, K)
    monkeypatch.delenv("RM_DEBUG_NO_ROW_TOPK")
    hip.reload_switches()
    check_lists(stored, fused, "RM_DEBUG_NO_ROW_TOPK=1")
    check_lists(fused, expected_lists(canonical(widen(bits, kind)), excl, K), "default")


# ---- 4. compaction under the worst order ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_compaction_under_the_worst_order(hip, kind, K):
    """rows ascending over 12,000 distinct finite values (positive patterns ascend with their values): every candidate beats the bound, so
    the buffer of 2,048 pairs fills again and again -- a step appends up to 1,024 pairs, as in the fp32 call"""
    m, n = 12, 12000
    bits = (1 + 700 * np.arange(m)[:, None] + np.arange(n)[None, :]).astype(np.uint16)
    W = widen(bits, kind)
    assert np.isfinite(W).all() and (np.diff(W, axis=1) > 0).all()
    excl = random_excl(m, n, 0.002, 51, empty=(0,))
    ids, sc, st = check_half_lists(hip, strided_bits(bits, n + 3, 2), kind, excl, K, "worst order K=%d" % K)
    assert ids[0].tolist() == list(range(n - 1, n - 1 - K, -1))


# ---- 5. ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_ties_are_ordered_by_item_id(hip, kind, K):
    m, n = 40, 5000
    rng = np.random.default_rng(61)
    values = narrow(np.linspace(-2, 2, 16), kind)
    assert np.unique(widen(values, kind)).shape[0] == 16
    bits = values[rng.integers(0, 16, (m, n))]
    excl = random_excl(m, n, 0.01, 62)
    ids, sc, st = check_half_lists(hip, strided_bits(bits, n + 3, 1), kind, excl, K, "16 values K=%d" % K)
    assert (st == 0).all()
    for u in range(m):                                                   # inside a run of equal scores the item ids ascend
        tied = np.flatnonzero(np.diff(sc[u]) == 0)
        assert tied.shape[0] >= K // 2 and (ids[u][tied + 1] > ids[u][tied]).all()
    same =np.full((m, n), narrow(np.array([0.25]), kind)[0], np.uint16)
    got = check_half_lists(hip, same, kind, excl, K, "all equal K=%d" % K)
    p, i = excl
    for u in (0, m - 1):
        assert got[0][u].tolist() == np.setdiff1d(np.arange(n), i[p[u]:p[u + 1]])[:K].tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_zeros_are_one_score(hip, kind):
    m, n, K = 20, 2500, 40
    rng = np.random.default_rng(64)
    bits = np.where(rng.random((m, n)) < 0.5, 0x0000, 0x8000).astype(np.uint16)
    minus_one = narrow(np.array([-1.0]), kind)[0]
    bits[m // 2:] = np.where(rng.random((m - m // 2, n)) < 0.9, bits[m // 2:], minus_one)       # (zeros lead these rows, -1 follows)
    bits[1] = 0x8000
    excl = random_excl(m, n, 0.01, 65, empty=(0,))
    ids, sc, st = check_half_lists(hip, strided_bits(bits, n + 3, 3), kind, excl, K, "zeros")
    assert (st == 0).all() and (sc == 0).all() and not np.signbit(sc).any()
    p, i = excl
    for u in (0, 1, 5):
        assert ids[u].tolist() == np.setdiff1d(np.arange(n), i[p[u]:p[u + 1]])[:K].tolist()


# ---- 6. non-finite candidates --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def metric_problem(K):
    """200 users x 300 items: planted_problem's edge users, three cold users (no train item) and a user whose test items are all train items"""
    m, n = 200, 300
    pr = planted_problem(m, n, 16, F32, 70, K)
    tep, tei, _ = pr["test"]
    rows = {u: (np.zeros(0, np.int32), tei[tep[u]:tep[u + 1]], None) for u in (20, 21, 22)}
    te = np.array([5, 17, 120, 250], np.int32)
    rows[23] = (np.union1d(te, np.arange(40, 60)).astype(np.int32), te, None)
    return replace_rows(pr, n, rows, F32)


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_candidates(hip, kind, poison):
    """lists: status 2 for the user with a non-finite CANDIDATE, nothing for the one with it at an excluded item; metrics: what the _f32
    entry says for W (the user NaN for a NaN; the factor call's validity rule for an infinity)"""
    m, n, K = 40, 3000, 10
    poison16 = narrow(np.array([poison]), kind)[0]
    bits0 = narrow(np.random.default_rng(71).standard_normal((m, n)), kind)
    excl = random_excl(m, n, 0.02, 72)
    clean = check_half_lists(hip, bits0, kind, excl, K, "clean")
    p, i = excl
    bits = bits0.copy()
    for u in (4, 11):
        bits[u, i[p[u] + 2]] = poison16
    hit = []
    for u in (9, 30):
        cand = np.setdiff1d(np.arange(n), i[p[u]:p[u + 1]])
        bits[u, cand[0] if u == 9 else cand[cand.shape[0] // 2]] = poison16
        hit.append(u)
    ids, sc, st = check_half_lists(hip, strided_bits(bits, n + 3, 7), kind, excl, K, "poison %r" % poison)
    others = np.setdiff1d(np.arange(m), hit)
    assert (st[others] == 0).all() and (st[hit] == 2).all() and (ids[hit] == -1).all() and np.isnan(sc[hit]).all()
    check_lists((ids[others], sc[others], st[others]), tuple(c[others] for c in clean), "the other users")
    # metrics
    pr = metric_problem(K)
    mm, nn = 200, 300
    mbits = narrow(np.random.default_rng(73).standard_normal((mm, nn)), kind)
    untouched = half_calc(hip, mbits, kind, pr["train"], pr["test"], K, cumulative=True)
    trp, tri = pr["train"]
    victims = [30, 31]
    for u in victims:
        cand = np.setdiff1d(np.arange(nn), tri[trp[u]:trp[u + 1]])
        mbits[u, cand[3]] = poison16
    for u in (40, 41, 42):                                             # at train items: ignored
        assert trp[u + 1] > trp[u]
        mbits[u, tri[trp[u]:trp[u + 1]]] = poison16
    got = half_calc(hip, strided_bits(mbits, nn + 3, 1), kind, pr["train"], pr["test"], K, cumulative=True)
    W = widen(mbits, kind)
    assert_all_bits(got, scores_calc(hip, W, pr["train"], pr["test"], K, cumulative=True, pad=3, dtype=F32), "%s poison %r: against the _f32 entry" % (kind, poison))
    rest = np.setdiff1d(np.arange(mm), victims)
    assert_all_bits({name: got[name][rest] for name in got}, {name: untouched[name][rest] for name in got}, "the other users")
    if poison != poison or poison > 0:
        assert all(np.isnan(got[name][victims]).all() for name in got)


# ---- 7. metrics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 10, 300])
@pytest.mark.parametrize("kind", KINDS)
def test_metrics(hip, oracle, kind, K):
    """all ten metrics, the default request (P, AP, NDCG) and `cumulative`, rows n + 3 apart, against the oracle on W and the _f32 entry"""
    pr = metric_problem(K)
    m, n = 200, 300
    bits = narrow(np.random.default_rng(80 + K).standard_normal((m, n)), kind)
    view = strided_bits(bits, n + 3, 1)
    W = widen(bits, kind)
    assert np.isfinite(W).all()
    for metrics, cum in ((ALL, False), (("p", "ap", "ndcg"), False), (ALL, True)):
        what = "%s K=%d %s cumulative=%s" % (kind, K, "all" if metrics is ALL else "default", cum)
        got = half_calc(hip, view, kind, pr["train"], pr["test"], K, metrics=metrics, cumulative=cum)
        want = oracle_on_scores(oracle, W, pr["train"], pr["test"], K, F32, metrics=metrics, cumulative=cum)
        assert_like_parity(got, want, what + ": against the oracle")
        f32 = scores_calc(hip, W, pr["train"], pr["test"], K, metrics=metrics, cumulative=cum, pad=3, dtype=F32)
        assert_all_bits(got, f32, what + ": against the _f32 entry")
    if K < 100:
        assert np.isfinite(got["P@K"]).sum() > m // 2 and np.isfinite(got["P@K"][[20, 21, 22]]).all()


# ---- 8. results depend neither on the batch size nor on the device list --------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_batches_and_shards_change_nothing(hip, monkeypatch, kind):
    m, n, K = 3000, 700, 10
    pr = planted_problem(m, n, 16, F32, 18, K)
    bits = narrow(np.random.default_rng(90).standard_normal((m, n)), kind)
    view = strided_bits(bits, n + 3, 1)
    excl = pr["train"]

    def both():
        return half_lists(hip, view, kind, excl, K), half_calc(hip, view, kind, pr["train"], pr["test"], K, cumulative=True)

    def same(got, what):
        check_lists(got[0], plain[0], what)
        assert_all_bits(got[1], plain[1], what)
    plain = both()
    W = widen(bits, kind)
    check_lists(plain[0], f32_lists(hip, W, excl, K), "unsharded: against the _f32 entry")
    assert_all_bits(plain[1], scores_calc(hip, W, pr["train"], pr["test"], K, cumulative=True, dtype=F32), "unsharded: against the _f32 entry")
    monkeypatch.setenv("RM_BATCH_USERS", "1024")
    same(both(), "batches of 1,024 users")
    monkeypatch.delenv("RM_BATCH_USERS")
    hip.set_devices([0, 0])
    try:
        same(both(), "two shards")
    finally:
        hip.set_devices([])


# ---- 9. / 10. the device entries and the Python surface: a process of its own (torch is loaded before the library) -------------------
def _child(mode):
    res = subprocess.run([sys.executable, os.path.join(HERE, "_scores_half_child.py"), mode], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_device_entries(hip):
    """torch device tensors in (300 x 5,000, rows n + 3 apart), lists (k_top on both paths) and metrics in device tensors out on a
    stream that is not the default one: the bits of the host entries"""
    done = _child("device")
    assert sorted(done) == sorted([kind, what] for kind in KINDS for what in ("lists 10", "lists 1024", "lists 1025", "metrics"))


def test_python_surface(hip):
    """CPU and GPU tensors of float16 / bfloat16 / float32 / float64 through recommend_topk_from_scores and
    calc_reco_metrics_from_scores: equal to the NumPy call on W (16-bit: float32 out) or on the array itself, `users=` included"""
    done = _child("python")
    assert sorted(done) == sorted([where, name] for where in ("cpu", "cuda") for name in ("float16", "bfloat16", "float32", "float64"))
