"""GPU: nothing of a request is lost between an entry and a batch.

Every scalar of the request takes a value that is not its default -- cumulative = 1, consider_cold_start = 0, min_items_pool = K + 5,
min_pos_test = 0, tie noise on with seed 12345 -- so that a field which does not reach HostRange::batch_call, or which a builder of
csrc/rm_lib.hip resets, changes a bit somewhere.  Each family is run (a) through its host entry in one batch, (b) through its host entry
in three batches and (c) through its device entry; the three must agree in every bit with each other and with the CPU oracle (ROC-AUC
against the oracle within an ulp, _util.roc_tol: x87 long double there).

The tie problem of tests/_requests.py (thousands of users whose lists only the noise orders), 2,500 users x 600 items x 16 factors,
K = 5: the factor path rounds RM_BATCH_USERS to 1,024 users, so 2,500 is the smallest m that gives three batches; the score path
takes RM_BATCH_USERS = 1000 as it is.  Two users without a train row and two with 8 candidates are planted, in the first and in the
last batch, for consider_cold_start and min_items_pool to decide somebody's outputs: test_metrics_from_factors asserts on the oracle
that each of cumulative, consider_cold_start, min_items_pool, the noise and the seed, put back to its default, changes a user's bits.
min_pos_test cannot: the reference clamps it to min(min_pos_test, 1) (quirk Q1 of oracle/recometrics_oracle.cpp) and a user without
a test item is NaN whatever it says, so 0 and 1 give the same outputs on every input."""
import ctypes as C
import functools

import numpy as np
import pytest

from _parity import NT, hip_calc
from _requests import replace_rows, tie_problem
from _util import assert_roc, assert_same_bits, same_bits
from test_hip_recommend import check_lists, expected_lists
from test_hip_recommend_scores import canonical
from test_hip_scores import oracle_on_scores, scores_calc

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
M, N, KF, K, K_TOP = 2500, 600, 16, 5, 7
KW = dict(cumulative=True, cold=False, min_items_pool=K + 5, min_pos_test=0)
NOISE = dict(noise=True, seed=12345)


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


class DeviceArrays:
    """device copies of NumPy arrays for the device entries, through the HIP runtime the library itself is linked against"""
    def __init__(self, hip):
        self.rt = hip.load()
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipFree.argtypes = [C.c_void_p]
        self.held = []

    def ok(self, rc):
        assert rc == 0, "HIP runtime error %d" % rc

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.rt.hipMalloc(C.byref(p), max(int(nbytes), 16)))
        self.held.append(p)
        return p.value

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        self.ok(self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1))             # hipMemcpyHostToDevice
        return p

    def get(self, p, shape, dtype):
        self.ok(self.rt.hipDeviceSynchronize())
        out = np.empty(shape, dtype)
        self.ok(self.rt.hipMemcpy(out.ctypes.data, p, out.nbytes, 2))         # hipMemcpyDeviceToHost
        return out

    def free(self):
        self.ok(self.rt.hipDeviceSynchronize())
        for p in self.held:
            self.ok(self.rt.hipFree(p))
        self.held = []


@pytest.fixture()
def dev(hip):
    d = DeviceArrays(hip)
    yield d
    d.free()


COLD_USERS, SMALL_POOL_USERS = (10, 2300), (11, 2301)


@functools.lru_cache(maxsize=None)
def problem(dtype):
    items = np.arange(N, dtype=np.int32)
    rows = {u: (np.zeros(0, np.int32), items[5:8], None) for u in COLD_USERS}
    rows.update({u: (items[8:], items[2:4], None) for u in SMALL_POOL_USERS})          # 8 candidates: 2 <= 8 < K + 5
    pr = replace_rows(tie_problem(dtype, M, N, KF), N, rows, dtype)
    A, B = np.ascontiguousarray(pr["A"], dtype), np.ascontiguousarray(pr["B"], dtype)
    trp, tri = [np.ascontiguousarray(x, np.int32) for x in pr["train"]]
    tep, tei = [np.ascontiguousarray(x, np.int32) for x in pr["test"][:2]]
    return pr, A, B, (trp, tri), (tep, tei, np.ascontiguousarray(pr["test"][2], dtype))


def metrics_on_device(hip, dev, dtype, source, train, test, noise_kw):
    """the ten metrics through a device entry; `source` = ("factors", A, B) or ("scores", S)"""
    from oracle.oracle import NAMES
    d_train = [dev.put(x) for x in train]
    d_test = [dev.put(x) for x in test]
    shapes = [(M, K)] * 8 + [(M,)] * 2
    outs = [dev.put(np.full(s, 7, dtype)) for s in shapes]
    if source[0] == "factors":
        hip.calc_metrics_device(dtype, dev.put(source[1]), KF, dev.put(source[2]), KF, M, N, KF, d_train[0], d_train[1], train[1].shape[0],
                                d_test[0], d_test[1], d_test[2], test[1].shape[0], K, outs, cumulative=True,
                                break_ties_with_noise=noise_kw["noise"], consider_cold_start=False, min_items_pool=K + 5, min_pos_test=0,
                                seed=noise_kw["seed"])
    else:
        hip.calc_metrics_scores_device(dtype, dev.put(source[1]), N, M, N, d_train[0], d_train[1], train[1].shape[0],
                                       d_test[0], d_test[1], d_test[2], test[1].shape[0], K, outs, cumulative=True,
                                       consider_cold_start=False, min_items_pool=K + 5, min_pos_test=0)
    return {NAMES[name]: dev.get(o, s, dtype) for name, o, s in zip(hip.METRIC_ORDER, outs, shapes)}


def in_three_batches(monkeypatch, capfd, users, call):
    """call() with RM_BATCH_USERS=users; the library's own trace of the host entry (RM_HOST_TRACE, on stderr) must speak of 3 batches"""
    monkeypatch.setenv("RM_BATCH_USERS", str(users))
    monkeypatch.setenv("RM_HOST_TRACE", "1")
    capfd.readouterr()
    got = call()
    trace = capfd.readouterr().err
    monkeypatch.delenv("RM_HOST_TRACE")
    monkeypatch.delenv("RM_BATCH_USERS")
    assert "rm host trace (3 batches" in trace, "RM_BATCH_USERS=%s did not give three batches: %s" % (users, trace[:200])
    return got


def assert_metrics(got, want, what, oracle=False):
    assert set(got) == set(want) and len(got) == 10, what
    for name in want:
        if oracle and name == "ROC_AUC":
            assert_roc(got[name], want[name], want[name].dtype, "%s: %s" % (what, name))
        else:
            assert_same_bits(got[name], want[name], "%s: %s" % (what, name))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_metrics_from_factors(hip, oracle, dev, monkeypatch, capfd, dtype):
    pr, A, B, train, test = problem(dtype)
    want = oracle.calc(A, B, train, test, K, dtype=dtype, nthreads=NT, **KW, **NOISE)
    for name, default, who in (("cold", True, COLD_USERS), ("min_items_pool", 2, SMALL_POOL_USERS), ("noise", False, None), ("seed", 1, None)):
        other = oracle.calc(A, B, train, test, K, dtype=dtype, nthreads=NT, **dict(dict(KW, **NOISE), **{name: default}))
        changed = ~np.all([same_bits(want[nm], other[nm]).reshape(M, -1).all(axis=1) for nm in want], axis=0)
        assert changed.any() and (who is None or changed[list(who)].all()), "%s changes no user of this problem" % name
    assert want["P@K"].shape == (M, K)                               # cumulative
    one = hip_calc(hip, A, B, train, test, K, dtype=dtype, **KW, **NOISE)
    assert_metrics(one, want, "host entry, one batch, against the oracle", oracle=True)
    three = in_three_batches(monkeypatch, capfd, 1024, lambda: hip_calc(hip, A, B, train, test, K, dtype=dtype, **KW, **NOISE))
    assert_metrics(three, one, "host entry, three batches")
    assert_metrics(metrics_on_device(hip, dev, dtype, ("factors", A, B), train, test, NOISE), one, "device entry")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_metrics_from_scores(hip, oracle, dev, monkeypatch, capfd, dtype):
    pr, A, B, train, test = problem(dtype)
    S = hip.debug_scores(A, B)
    want = oracle_on_scores(oracle, S, train, test, K, dtype, **KW)
    one = scores_calc(hip, S, train, test, K, dtype=dtype, **KW)
    assert_metrics(one, want, "host entry, one batch, against the oracle", oracle=True)
    three = in_three_batches(monkeypatch, capfd, 1000, lambda: scores_calc(hip, S, train, test, K, dtype=dtype, **KW))
    assert_metrics(three, one, "host entry, three batches")
    assert_metrics(metrics_on_device(hip, dev, dtype, ("scores", S), train, test, None), one, "device entry")


def lists_on_device(hip, dev, dtype, source, excl):
    d_excl = [dev.put(x) for x in excl] if excl is not None else [0, 0]
    nnz = excl[1].shape[0] if excl is not None else 0
    idx, sc, st = dev.put(np.full((M, K_TOP), 77, np.int32)), dev.put(np.full((M, K_TOP), 7, dtype)), dev.put(np.full(M, 77, np.int32))
    if source[0] == "factors":
        hip.recommend_device(dtype, dev.put(source[1]), KF, dev.put(source[2]), KF, M, N, KF, d_excl[0], d_excl[1], nnz, K_TOP, idx, sc, st)
    else:
        hip.recommend_scores_device(dtype, dev.put(source[1]), N, M, N, d_excl[0], d_excl[1], nnz, K_TOP, idx, sc, st)
    return dev.get(idx, (M, K_TOP), np.int32), dev.get(sc, (M, K_TOP), dtype), dev.get(st, (M,), np.int32)


@pytest.mark.parametrize("family", ["factors", "scores"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lists(hip, oracle, dev, monkeypatch, capfd, dtype, family):
    pr, A, B, excl, _ = problem(dtype)
    if family == "factors":
        S = oracle.scores(A, B, dtype=dtype)
        source, batch = ("factors", A, B), 1024
        host = lambda x: hip.recommend(A, KF, B, KF, None if x is None else x[0], None if x is None else x[1], K_TOP)
    else:
        S = canonical(hip.debug_scores(A, B))
        source, batch = ("scores", S), 1000
        host = lambda x: hip.recommend_scores(S, N, None if x is None else x[0], None if x is None else x[1], K_TOP)
    for x, what in ((excl, "an exclusion matrix"), (None, "no exclusion matrix")):
        want = expected_lists(S, x, K_TOP)
        check_lists(host(x), want, "%s: host entry, one batch" % what)
        check_lists(in_three_batches(monkeypatch, capfd, batch, lambda: host(x)), want, "%s: host entry, three batches" % what)
        check_lists(lists_on_device(hip, dev, dtype, source, x), want, "%s: device entry" % what)
