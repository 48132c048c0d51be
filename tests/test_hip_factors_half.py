"""GPU: metrics and top-K lists from factor matrices in IEEE binary16 ("f16") / bfloat16 ("bf16") --
include/recometrics_hip_half_factors.h, and `A` / `B` as torch.Tensors.

The contract is one sentence: for 16-bit matrices A and B, let WA and WB be the fp32 matrices with the same elements exactly; every entry
returns what its _f32 counterpart returns for WA, WB.  WA and WB are formed on the CPU (`widen` of tests/test_hip_scores_half.py) and the
expected values come from code that is not under test:
  lists    `expected_lists` of tests/test_hip_recommend.py (NumPy lexsort) on oracle.scores(WA, WB);
  metrics  oracle.calc(WA, WB), by `assert_like_parity` of tests/test_hip_scores.py: bitwise, ROC-AUC within _util.roc_tol;
  both     the _f32 entry on WA, WB, bit for bit (`assert_all_bits`, `check_lists`).
No tolerance is introduced here."""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _parity import NT, hip_calc
from _requests import ALL, DEFAULT, edge_problem, equal_problem, runs_problem, tie_problem
from _warm_bounds import hintable, lists_of
from test_hip_entry_fields import DeviceArrays
from test_hip_recommend import check_lists, expected_lists
from test_hip_scores import assert_all_bits, assert_like_parity
from test_hip_scores_half import NAN16, csr_of, narrow, non_finite, widen

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = ("f16", "bf16")
HERE = os.path.dirname(os.path.abspath(__file__))
ONE = {"f16": 0x3c00, "bf16": 0x3f80}                 # the pattern of 1.0


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


@pytest.fixture()
def dev(hip):
    d = DeviceArrays(hip)
    yield d
    d.free()


@contextlib.contextmanager
def switches(monkeypatch, env):
    """the library under these switches (tests/conftest.py reloads them with the environment), and without them again afterwards"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    try:
        yield
    finally:
        for name in env:
            monkeypatch.delenv(name)


# ---- the entries by host arrays ------------------------------------------------------------------------------------------------------
def as_argument(bits, kind):
    """what the binding's 16-bit wrappers take: a float16 array, or bf16 patterns as uint16 (strides kept)"""
    return bits.view(np.float16) if kind == "f16" else bits


def half_lists(hip, A, B, kind, excl, K, scores=True):
    keep = A.copy(), B.copy()
    got = hip.recommend_half(as_argument(A, kind), A.strides[0] // 2, as_argument(B, kind), B.strides[0] // 2,
                             None if excl is None else excl[0], None if excl is None else excl[1], K, scores)
    assert (A == keep[0]).all() and (B == keep[1]).all(), "the caller's factors were modified"
    return got


def f32_lists(hip, WA, WB, excl, K):
    return hip.recommend(WA, WA.shape[1], WB, WB.shape[1], None if excl is None else excl[0], None if excl is None else excl[1], K)


def half_calc(hip, A, B, kind, train, test, k, metrics=ALL, cumulative=False, noise=False, cold=True, min_items_pool=2, min_pos_test=1, seed=1, **_):
    from oracle.oracle import NAMES
    trp, tri = [np.ascontiguousarray(x, dtype=np.int32) for x in train[:2]]
    tep, tei = [np.ascontiguousarray(x, dtype=np.int32) for x in test[:2]]
    tev = np.ascontiguousarray(test[2], dtype=F32) if len(test) > 2 and test[2] is not None else np.ones(tei.shape[0], F32)
    want = {name: (name in metrics) for name in hip.METRIC_ORDER}
    outs = hip.calc_metrics_half(as_argument(A, kind), A.strides[0] // 2, as_argument(B, kind), B.strides[0] // 2, trp, tri, tep, tei, tev, k, want,
                                 cumulative, noise, cold, min_items_pool, min_pos_test, 1, seed)
    assert all(o.dtype == F32 for o in outs)
    return {NAMES[name]: arr for name, arr in zip(hip.METRIC_ORDER, outs) if want[name]}


class Narrowed:
    """a problem with its factors narrowed to `kind`: the patterns, and the fp32 matrices with exactly their values"""
    def __init__(self, pr, kind, bits=None):
        self.kind, self.A, self.B = (kind,) + (bits or (narrow(pr["A"], kind), narrow(pr["B"], kind)))
        self.WA, self.WB = widen(self.A, kind), widen(self.B, kind)
        self.train = tuple(np.ascontiguousarray(x, np.int32) for x in pr["train"][:2])
        self.test = tuple(np.ascontiguousarray(x, np.int32) for x in pr["test"][:2]) + (np.ascontiguousarray(pr["test"][2], F32),)
        self.m, self.n, self.k = self.A.shape[0], self.B.shape[0], self.A.shape[1]


def check_metrics(hip, oracle, p, K, what, against_oracle=True, **kw):
    """the 16-bit host entry against the _f32 entry on (WA, WB) in every bit, and against the oracle by the suite's rule"""
    got = half_calc(hip, p.A, p.B, p.kind, p.train, p.test, K, **kw)
    assert_all_bits(got, hip_calc(hip, p.WA, p.WB, p.train, p.test, K, dtype=F32, **kw), "%s %s: against the _f32 entry" % (p.kind, what))
    if against_oracle:
        okw = {name: v for name, v in kw.items() if name != "metrics"}
        want = oracle.calc(p.WA, p.WB, p.train, p.test, K, metrics=kw.get("metrics", ALL), dtype=F32, nthreads=NT, **okw)
        assert_like_parity(got, want, "%s %s: against the oracle" % (p.kind, what))
    return got


def check_half_lists(hip, oracle, p, K, what, excl="train"):
    excl = p.train if excl == "train" else excl
    got = half_lists(hip, p.A, p.B, p.kind, excl, K)
    assert got[1].dtype == F32
    check_lists(got, expected_lists(oracle.scores(p.WA, p.WB, dtype=F32), excl, K), "%s %s: against NumPy" % (p.kind, what))
    check_lists(got, f32_lists(hip, p.WA, p.WB, excl, K), "%s %s: against the _f32 entry" % (p.kind, what))
    return got


# ---- the entries by device pointers --------------------------------------------------------------------------------------------------
def place(dev, bits, ld, off):
    """(device address of bits[0, 0], ld): rows `ld` elements apart, the first `off` elements past a 16-byte boundary, NaN between them"""
    m, k = bits.shape
    raw = np.full(m * ld + off + 8, NAN16, np.uint16)
    raw[off:off + m * ld].reshape(m, ld)[:, :k] = bits
    base = dev.put(raw)
    assert base % 16 == 0
    return base + 2 * off, ld


class Split:
    def __init__(self, dev, train, test):
        self.train, self.test = [dev.put(x) for x in train], [dev.put(x) for x in test]
        self.nnz_train, self.nnz_test = train[1].shape[0], test[1].shape[0]


def metrics_dev(hip, dev, kind, A, B, m, n, k, sp, K, stream=0, **kw):
    """all ten metrics through rm_calc_metrics_dev_{f16,bf16} (or, kind F32, _f32): A = (address, lda), B = (address, ldb)"""
    from oracle.oracle import NAMES
    outs = [dev.put(np.full(m, 7, F32)) for _ in hip.METRIC_ORDER]
    entry = hip.calc_metrics_device if kind is F32 else hip.calc_metrics_half_device
    entry(kind, A[0], A[1], B[0], B[1], m, n, k, sp.train[0], sp.train[1], sp.nnz_train, sp.test[0], sp.test[1], sp.test[2], sp.nnz_test, K, outs,
          stream=stream, **kw)
    return {NAMES[name]: dev.get(o, (m,), F32) for name, o in zip(hip.METRIC_ORDER, outs)}


def lists_dev(hip, dev, kind, A, B, m, n, k, excl, nnz, K):
    idx, sc, st = dev.put(np.full((m, K), 77, np.int32)), dev.put(np.full((m, K), 7, F32)), dev.put(np.full(m, 77, np.int32))
    hip.recommend_half_device(kind, A[0], A[1], B[0], B[1], m, n, k, excl[0], excl[1], nnz, K, idx, sc, st)
    return dev.get(idx, (m, K), np.int32), dev.get(sc, (m, K), F32), dev.get(st, (m,), np.int32)


# ---- 1. factor-count edges -----------------------------------------------------------------------------------------------------------
FACTOR_COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 130, 264)


@functools.lru_cache(maxsize=None)
def iid(m, n, k, seed, mean_c=20):
    from recometrics_amd.synth import make_problem
    return make_problem(m, n, k, F32, mean_c=mean_c, seed=seed)


@pytest.mark.parametrize("k", FACTOR_COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_factor_count_edges(hip, oracle, dev, kind, k):
    """70 x 700: more than one item tile, the last one ragged; 264 factors take k_pack_items.  The host entries stage dense rows (16-byte
    loads where 2 k is a multiple of 16); the device entries get lda = k + 3, ldb = k + 5 and every 2-byte phase of the first element"""
    p = Narrowed(iid(70, 700, k, 100 + k), kind)
    top10 = check_half_lists(hip, oracle, p, 10, "k=%d k_top=10" % k)
    check_half_lists(hip, oracle, p, p.n, "k=%d k_top=n" % k)              # every candidate's score: every score of the sweep
    dense = check_metrics(hip, oracle, p, 10, "k=%d all ten" % k)
    sp = Split(dev, p.train, p.test)
    for off in (1, 3, 4, 7):
        A, B = place(dev, p.A, k + 3, off), place(dev, p.B, k + 5, off)
        got = lists_dev(hip, dev, kind, A, B, p.m, p.n, k, sp.train, sp.nnz_train, 10)
        check_lists(got, top10, "%s k=%d off=%d: device lists against the dense host call" % (kind, k, off))
        got = metrics_dev(hip, dev, kind, A, B, p.m, p.n, k, sp, 10)
        assert_all_bits(got, dense, "%s k=%d off=%d: device metrics against the dense host call" % (kind, k, off))


# ---- 2. / 3. every pattern widens exactly ---------------------------------------------------------------------------------------------
ALL_PATTERNS = np.arange(65536, dtype=np.uint16)


@pytest.mark.parametrize("kind", KINDS)
def test_every_pattern_widens_exactly_in_b(hip, kind):
    """k = 1, every user's factor 1.0: the score of item i is widen(i).  Users 0 and 1 exclude exactly the NaN / +-Inf patterns, user 2
    nothing (status 2), user 3 everything (status 1) -- the rows of test_every_value_widens_exactly"""
    A, B = np.full((4, 1), ONE[kind], np.uint16), ALL_PATTERNS.reshape(-1, 1).copy()
    bad = np.flatnonzero(non_finite(ALL_PATTERNS, kind)).astype(np.int32)
    excl = csr_of([bad, bad, np.zeros(0, np.int32), np.arange(65536, dtype=np.int32)])
    WA, WB = widen(A, kind), widen(B, kind)
    with np.errstate(invalid="ignore"):
        S = (WA * WB.T + F32(0)).astype(F32)                                # one fma from +0: the product itself, -0 as +0
    got = half_lists(hip, A, B, kind, excl, 10)
    check_lists(got, expected_lists(S, excl, 10), "%s all patterns in B: against NumPy" % kind)
    check_lists(got, f32_lists(hip, WA, WB, excl, 10), "%s all patterns in B: against the _f32 entry" % kind)
    assert got[2].tolist() == [0, 0, 2, 1]
    top = np.sort(widen(ALL_PATTERNS[~non_finite(ALL_PATTERNS, kind)], kind))[::-1][:10]
    assert (got[1][0] == top).all() and (got[1][1] == top).all()


@pytest.mark.parametrize("kind", KINDS)
def test_every_pattern_widens_exactly_in_a(hip, kind):
    """k = 1, every pattern a user, eight items of factor 1.0: through k_pack_users and k_absmax (lists), and -- a test row of one item
    per user, K = 1, all ten metrics -- through FlatDot"""
    A, B = ALL_PATTERNS.reshape(-1, 1).copy(), np.full((8, 1), ONE[kind], np.uint16)
    WA, WB = widen(A, kind), widen(B, kind)
    ids, sc, st = half_lists(hip, A, B, kind, None, 1)
    finite = ~non_finite(ALL_PATTERNS, kind)
    assert (st == np.where(finite, 0, 2)).all()
    assert (sc[finite, 0].view(np.uint32) == (WA[finite, 0] + F32(0)).view(np.uint32)).all() and (ids[finite, 0] == 0).all()
    check_lists((ids, sc, st), f32_lists(hip, WA, WB, None, 1), "%s all patterns in A: against the _f32 entry" % kind)
    m = 65536
    train = (np.zeros(m + 1, np.int32), np.zeros(0, np.int32))
    test = (np.arange(m + 1, dtype=np.int32), (np.arange(m) % 8).astype(np.int32), np.ones(m, F32))
    got = half_calc(hip, A, B, kind, train, test, 1)
    assert_all_bits(got, hip_calc(hip, WA, WB, train, test, 1, dtype=F32), "%s all patterns in A, metrics: against the _f32 entry" % kind)


# ---- 4. subnormals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_subnormal_factors_are_not_flushed(hip, kind):
    """user factors that are subnormal patterns of both signs, item factors exact powers of two: 6 x 3,000 x 8.  f16: every product and
    every partial sum is exact in fp32 (multiples of 2^-27 below 2^-10), so NumPy's float64 product is the chain's result, and the
    widened values are fp32 NORMALS -- whatever the matrix instruction does with fp32 subnormals.  bf16 subnormals are fp32 subnormals:
    against the _f32 entry only"""
    frac = 0x3ff if kind == "f16" else 0x7f
    m, n, k, K = 6, 3000, 8, 100
    rng = np.random.default_rng(4)
    A = (rng.integers(1, frac + 1, (m, k)) | (rng.integers(0, 2, (m, k)) << 15)).astype(np.uint16)
    B = narrow(np.ldexp(1.0, rng.integers(-3, 4, (n, k))).astype(F32) * rng.choice(np.array([-1.0, 1.0], F32), (n, k)), kind)
    WA, WB = widen(A, kind), widen(B, kind)
    assert (np.abs(WA) < (2.0 ** -14 if kind == "f16" else 2.0 ** -126)).all() and (WA != 0).all() and (np.frexp(np.abs(WB))[0] == 0.5).all()
    excl = csr_of([np.sort(rng.permutation(n)[:30]).astype(np.int32) for _ in range(m)])
    got = half_lists(hip, A, B, kind, excl, K)
    check_lists(got, f32_lists(hip, WA, WB, excl, K), "%s subnormal factors: against the _f32 entry" % kind)
    if kind == "f16":
        S = (WA.astype(np.float64) @ WB.astype(np.float64).T).astype(F32)
        assert (S.astype(np.float64) == WA.astype(np.float64) @ WB.astype(np.float64).T).all()
        check_lists(got, expected_lists(S + F32(0), excl, K), "f16 subnormal factors: against NumPy")
        ids, sc, st = got
        assert (st == 0).all() and (sc[:, 0] > 0).all() and (np.diff(sc, axis=1) <= 0).all() and (sc[:, 0] > sc[:, -1]).all()
        assert (ids[:, :K] != np.arange(K)).any(axis=1).all(), "flushed: the list is the smallest item ids"


# ---- 5. overflow and non-finite factors ----------------------------------------------------------------------------------------------
def poisoned_problem(m, n, k, seed):
    """bf16.  Users 0-2 and items 0-3 hold factors of about 2^100: their chains overflow to +-Inf.  Items R1 hold NaN / +-Inf patterns and
    are train items of everybody; items R2 hold them too and are train items of the even users only -- the odd users meet them as
    candidates.  `clean`: the same problem with ordinary values in R1 and R2"""
    rng = np.random.default_rng(seed)
    A, B = narrow(rng.standard_normal((m, k)), "bf16"), narrow(rng.standard_normal((n, k)), "bf16")
    big = narrow(np.ldexp(rng.choice(np.array([-1.0, 1.0]), (4, k)), 100).astype(F32), "bf16")
    A[:3], B[:4] = big[:3], big
    R1, R2 = np.array([5, n // 2, n - 1]), np.array([9, n // 3])
    clean = B.copy()
    B[R1] = np.array([0x7fc0, 0x7f80, 0xff80], np.uint16)[:, None]          # NaN, +Inf, -Inf
    B[R2] = np.array([0xffc1, 0x7f80], np.uint16)[:, None]
    ordinary = np.setdiff1d(np.arange(n), np.concatenate([R1, R2]))
    TR, TE = [], []
    for u in range(m):
        pick = rng.permutation(ordinary)
        TE.append(np.sort(pick[:5]))
        TR.append(np.sort(np.concatenate([pick[5:25], R1] + ([R2] if u % 2 == 0 else []))))
    train, test = csr_of(TR), csr_of(TE) + (np.ones(5 * m, F32),)
    return tuple(Narrowed(dict(train=train, test=test), "bf16", bits=(A, b)) for b in (B, clean))


def test_overflow_and_non_finite_factors_lists(hip, oracle):
    p, clean = poisoned_problem(40, 3000, 16, 50)
    assert non_finite(p.B, "bf16").any(axis=1).sum() == 5 and not non_finite(clean.B, "bf16").any() and np.isinf(oracle.scores(p.WA[:3], clean.WB[:4])).all()
    got = check_half_lists(hip, oracle, p, 10, "poisoned lists")
    ids, sc, st = got
    met = np.arange(p.m) % 2 == 1
    assert (st[met] == 2).all() and (st[:3] == 2).all(), st.tolist()
    quiet = ~met & (np.arange(p.m) >= 3)
    assert quiet.any() and (st[quiet] == 0).all()
    want = half_lists(hip, clean.A, clean.B, "bf16", clean.train, 10)
    check_lists(tuple(x[quiet] for x in got), tuple(x[quiet] for x in want), "users that meet no such value: the clean problem's lists")


def test_overflow_and_non_finite_factors_metrics(hip, oracle):
    p, clean = poisoned_problem(200, 300, 16, 51)
    got = check_metrics(hip, oracle, p, 10, "poisoned metrics")
    met = np.arange(p.m) % 2 == 1
    assert np.isnan(got["P@K"][met]).all() and np.isnan(got["P@K"][:3]).all()
    quiet = ~met & (np.arange(p.m) >= 3)
    want = half_calc(hip, clean.A, clean.B, "bf16", clean.train, clean.test, 10)
    assert np.isfinite(want["P@K"][quiet]).all()
    assert_all_bits({name: x[quiet] for name, x in got.items()}, {name: x[quiet] for name, x in want.items()}, "users that meet no such value")


# ---- 6. metrics on the edge users ----------------------------------------------------------------------------------------------------
NOISE = dict(noise=True, seed=7)
REQUESTS = (("all ten", dict(metrics=ALL)), ("the default three", dict(metrics=DEFAULT)), ("cumulative", dict(metrics=ALL, cumulative=True)))
PATHS = (("", {}), ("scores by slot", {"RM_DEBUG_NO_POS_FLAT": "1"}), ("two item splits", {"RM_DEBUG_SPLITS": "2,1,3"}))


@pytest.mark.parametrize("K", [1, 10, 300])
@pytest.mark.parametrize("kind", KINDS)
def test_metrics_on_the_edge_users(hip, oracle, monkeypatch, kind, K):
    """edge_problem (129 x 1,000 x 16) with narrowed factors: tie noise off and on, through k_pos_scores_flat, k_pos_scores and a sweep
    over two item ranges"""
    p = Narrowed(edge_problem(F32, K), kind)
    plain = oracle.calc(p.WA, p.WB, p.train, p.test, K, dtype=F32, nthreads=NT)
    assert np.isfinite(plain["P@K"]).sum() > p.m // 2, "more than half of the users are evaluated"
    assert np.isnan(plain["P@K"][[0, 6]]).all(), "no test item; a train row that is the whole catalogue"
    for path, env in PATHS:
        with switches(monkeypatch, env):
            for request, kw in REQUESTS:
                for noise in ({}, NOISE):
                    got = check_metrics(hip, oracle, p, K, "K=%d %s %s %s" % (K, request, path, noise), **kw, **noise)
            if "RM_DEBUG_SPLITS" in env:
                assert hip.timings()["item_splits"] == 2
    assert np.isnan(got["P@K"][[0, 6]]).all()


# ---- 7. ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("problem", [tie_problem, equal_problem, runs_problem], ids=["ties", "equal", "runs"])
@pytest.mark.parametrize("kind", KINDS)
def test_ties(hip, oracle, kind, problem, K):
    p = Narrowed(problem(F32), kind)
    check_metrics(hip, oracle, p, K, "%s K=%d" % (problem.__name__, K), against_oracle=False)
    ids, sc, st = got = half_lists(hip, p.A, p.B, kind, p.train, K)
    check_lists(got, f32_lists(hip, p.WA, p.WB, p.train, K), "%s %s K=%d: lists against the _f32 entry" % (kind, problem.__name__, K))
    tied = (sc[:, 1:] == sc[:, :-1]) & (st == 0)[:, None]
    assert tied.any() and (ids[:, 1:][tied] > ids[:, :-1][tied]).all(), "inside a run of equal scores the ids ascend"


# ---- 8. k_top paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 10, 20, 21, 64, 256, 257, 1000])
@pytest.mark.parametrize("kind", KINDS)
def test_k_top_paths(hip, oracle, kind, K):
    check_half_lists(hip, oracle, Narrowed(iid(48, 6000, 24, 33, mean_c=60), kind), K, "k_top=%d" % K)


# ---- 9. warm bounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_warm_bounds_on_the_kept_split(hip, oracle, dev, monkeypatch, kind):
    """two device metric calls on one kept split (the first problem's), the second with other 16-bit factors: it takes bounds from the first call's lists
    (rm_get_timings out[11], for exactly the users tests/_warm_bounds.py accepts) and computes what it computes without them"""
    K = 10
    first, second = Narrowed(iid(300, 700, 16, 9, mean_c=60), kind), Narrowed(iid(300, 700, 16, 10, mean_c=60), kind)
    sp = Split(dev, first.train, first.test)
    placed = [(place(dev, p.A, p.k, 0), place(dev, p.B, p.k, 0)) for p in (first, second)]

    def two_calls():
        out = []
        for p, (A, B) in zip((first, second), placed):
            out.append((metrics_dev(hip, dev, kind, A, B, p.m, p.n, p.k, sp, K), hip.timings()["split_reused"], hip.hinted_users()))
        return out
    hip.load().rm_release_workspace()                                      # (no split, no lists of an earlier test)
    warm = two_calls()
    ids = lists_of(oracle.scores(first.WA, first.WB, dtype=F32), first.train[0], first.train[1], K)
    expect = int(hintable(ids, first.n, first.train[0], first.train[1], first.test[0]).sum())
    assert [w[1] for w in warm] == [0, 1] and warm[0][2] == 0 and warm[1][2] == expect > 0, ([w[1:] for w in warm], expect)
    with switches(monkeypatch, {"RM_DEBUG_NO_WARM_BOUNDS": "1"}):
        hip.load().rm_release_workspace()
        cold = two_calls()
    assert [c[2] for c in cold] == [0, 0]
    for i, p in enumerate((first, second)):
        assert_all_bits(warm[i][0], cold[i][0], "%s call %d: with bounds against without" % (kind, i))
        assert_all_bits(warm[i][0], hip_calc(hip, p.WA, p.WB, first.train, first.test, K, dtype=F32), "%s call %d: against the _f32 entry" % (kind, i))


# ---- 10. batches and shards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_batches_and_shards_change_nothing(hip, oracle, monkeypatch, kind):
    p = Narrowed(iid(3000, 700, 16, 77), kind)
    call = lambda: half_calc(hip, p.A, p.B, kind, p.train, p.test, 10, **NOISE)
    plain = call()
    assert_all_bits(plain, hip_calc(hip, p.WA, p.WB, p.train, p.test, 10, dtype=F32, **NOISE), "%s one call: against the _f32 entry" % kind)
    with switches(monkeypatch, {"RM_BATCH_USERS": "1024"}):
        assert_all_bits(call(), plain, "%s three batches against one call" % kind)
    before = hip.get_devices()
    try:
        hip.set_devices([0, 0])
        assert_all_bits(call(), plain, "%s two shards against one call" % kind)
        with switches(monkeypatch, {"RM_BATCH_USERS": "1024"}):
            assert_all_bits(call(), plain, "%s two shards of two batches against one call" % kind)
    finally:
        hip.set_devices(before)


# ---- 11. device entries on a stream of the caller's, and the Python surface ------------------------------------------------------------
def test_the_python_surface_with_torch_loaded_first():
    """a fresh interpreter that imports torch before the library (tests/_factors_half_child.py): device tensors on a non-default stream
    through the device entries, CPU and GPU tensors of all four dtypes through calc_reco_metrics and recommend_topk"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("RM_")}
    res = subprocess.run([sys.executable, os.path.join(HERE, "_factors_half_child.py")], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    report = json.loads(res.stdout.strip().splitlines()[-1])
    assert report["ok"] and report["checked"] >= 40, report
