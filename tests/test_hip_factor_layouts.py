"""GPU: factor matrices with a row stride or an unaligned base give what dense, aligned ones give -- in every bit of every entry.

The C-ABI takes `lda` / `ldb` and any pointer.  The host entries compact the caller's rows into dense, aligned staging before a kernel
sees them, so only the DEVICE entries hand a stride or an unaligned base to a kernel: k_absmax (its flat branch wants ld == k and an
aligned base; the answer decides whether the sweep may skip its NaN scan), the packing kernels (k_pack_items, k_pack_items_tile,
k_pack_users, k_pack_items64, k_pack_users64), k_pos_scores / k_pos_scores_flat (16-byte loads when `(base | ld * sizeof(T)) & 15`
is 0) and chain_dot.  The host code that steps through A by `lda` is reached too: the fp64 tie-noise slices of a device call, the exact
fp32 pass over a subset of the users, the sample seed's pack of the first items, and the host entry's own `h.A + (u0 + b0) * h.lda`
once there is more than one batch or shard.

The layouts and the pairs (layout of A, layout of B) are tests/_layouts.py's; tests/test_factor_layouts_cpu.py proves them.  Every
element of a buffer that is not a factor holds a poison.  Two expectations hold for every strided call:
  (a) its outputs equal the same entry's outputs on the (D, D) copy of the same factors in every bit, ROC-AUC included -- the same
      arithmetic on the same device;
  (b) its outputs equal the oracle's on the compacted arrays by the suite's rule: bit for bit, ROC-AUC by assert_roc (_util.roc_tol).
No tolerance is introduced here.  Where max |x| is looked at, the gaps hold the largest finite magnitudes and the sweep launch ledger
(rm_debug_sweep_launched) must name exactly the rows the (D, D) call launched: a k_absmax that read a gap would move the call to a
check_nan row, which computes the same outputs.

Problem S: the split and the factors of tests/test_hip_sweep_rows.py (200 users x 1,237 items, test rows of 1 to 63 items, five
streamed users, three without test items).  Problem T: the tie problem of tests/test_hip_entry_fields.py (2,500 users x 600 items x 16
factors: three host batches, thousands of users inside the fp32 noise zone)."""
import contextlib
import functools
import re

import numpy as np
import pytest

import _layouts as lay
import test_hip_entry_fields as T
from _parity import NT, hip_calc
from _requests import ALL, TOPK8
from _util import assert_roc, assert_same_bits
from test_factor_layouts_cpu import K_SPECIAL, SPECIAL_FACTORS, special_problem
from test_hip_entry_fields import DeviceArrays, in_three_batches
from test_hip_recommend import check_lists, expected_lists
from test_hip_sweep_rows import DTYPE, M_USERS, N_ITEMS, launched_anywhere, problem, table, want_calc, want_lists  # noqa: F401 (table: a fixture)

pytestmark = pytest.mark.gpu
HOST_TRACE = re.compile(r"rm host trace \((\d+) batches")
K_TOP = 7
S_FACTORS = (("f32", 16), ("f32", 13), ("f32", 260), ("f64", 16), ("f64", 13))
LIST_FACTORS = (("f32", 16), ("f32", 13), ("f64", 16), ("f64", 13))
TIE_PAIRS = (("RO", "D"), ("D", "RO"), ("RA", "R1"), ("O1", "O1"))
HOST_PAIRS = (("R1", "RA"), ("RO", "RO"))


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


@pytest.fixture
def device_list(hip):
    """the process's device list as the test found it, whatever the test did to it and however it ended"""
    before = hip.get_devices()
    yield
    hip.set_devices(before)


@contextlib.contextmanager
def switches(monkeypatch, hip, env):
    """the library under these switches, and without them again afterwards"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    hip.reload_switches()
    try:
        yield
    finally:
        for name in env:
            monkeypatch.delenv(name)
        hip.reload_switches()


def on_device(dev, X, name, poison):
    """(device address of X[0, 0], leading dimension) of a copy of X in layout `name`: one upload of the raw buffer, pointer arithmetic"""
    V, raw, at = lay.place_as(X, name, poison[lay.PREC[np.dtype(X.dtype)]])
    base = dev.put(raw)
    assert base % 16 == 0 and raw.ctypes.data % 16 == 0
    p = base + at * raw.itemsize
    assert p % 16 == V.ctypes.data % 16
    return p, V.strides[0] // raw.itemsize


class Split:
    """device copies of a train / test split, uploaded once per test"""
    def __init__(self, dev, train, test):
        self.train, self.test = [dev.put(x) for x in train], [dev.put(x) for x in test]
        self.nnz_train, self.nnz_test = train[1].shape[0], test[1].shape[0]


def metrics_dev(hip, dev, dtype, A, B, m, n, k, sp, K, request, **kw):
    """a device metric entry, cumulative: A = (address, lda), B = (address, ldb); {name: array} of the metrics of `request`"""
    from oracle.oracle import NAMES
    shapes = [(m, K)] * 8 + [(m,)] * 2
    outs = [dev.put(np.full(s, 7, dtype)) if name in request else 0 for name, s in zip(hip.METRIC_ORDER, shapes)]
    hip.calc_metrics_device(dtype, A[0], A[1], B[0], B[1], m, n, k, sp.train[0], sp.train[1], sp.nnz_train, sp.test[0], sp.test[1], sp.test[2],
                            sp.nnz_test, K, outs, cumulative=True, **kw)
    return {NAMES[name]: dev.get(o, s, dtype) for name, o, s in zip(hip.METRIC_ORDER, outs, shapes) if o}


def lists_dev(hip, dev, dtype, A, B, m, n, k, excl, nnz):
    idx, sc, st = dev.put(np.full((m, K_TOP), 77, np.int32)), dev.put(np.full((m, K_TOP), 7, dtype)), dev.put(np.full(m, 77, np.int32))
    hip.recommend_device(dtype, A[0], A[1], B[0], B[1], m, n, k, excl[0], excl[1], nnz, K_TOP, idx, sc, st)
    return dev.get(idx, (m, K_TOP), np.int32), dev.get(sc, (m, K_TOP), dtype), dev.get(st, (m,), np.int32)


def assert_same_outputs(got, want, what):
    """(a): every bit, ROC-AUC included"""
    assert set(got) == set(want), what
    for name in want:
        assert_same_bits(got[name], want[name], "%s: %s" % (what, name))


def assert_oracle(got, want, dtype, what):
    """(b): the suite's rule against the oracle"""
    assert set(got) == set(want), what
    for name in want:
        if name == "ROC_AUC":
            assert_roc(got[name], want[name], dtype, "%s: %s" % (what, name))
        else:
            assert_same_bits(got[name], want[name], "%s: %s" % (what, name))


def ledger_call(hip, table, call):
    """call() and the rows of the sweep tables it launched: {(prec, key): launches}"""
    hip.load().rm_debug_sweep_launched_reset()
    got = call()
    return got, launched_anywhere(hip, table)


# ---- 3a. the device metric entry on S -------------------------------------------------------------------------------------------------
RUNS = (("all ten, K = 5", ALL, 5, {}),
        ("all ten, K = 40 (lane buffers)", ALL, 40, {}),
        ("top-K eight, K = 5 (the auc = 0 kernels)", TOPK8, 5, {}),
        ("all ten, K = 40, a sample seed of 64 items", ALL, 40, {"RM_DEBUG_SAMPLE_SEED": "64"}),
        ("all ten, K = 5, the positives' scores by slot", ALL, 5, {"RM_DEBUG_NO_POS_FLAT": "1"}))


@pytest.mark.parametrize("prec,factors", S_FACTORS, ids=["%s-%d" % pf for pf in S_FACTORS])
def test_device_metric_entry(hip, oracle, dev, table, monkeypatch, prec, factors):
    """Every pair through rm_calc_metrics_dev_*, the gaps at the largest finite magnitudes.  Factor counts: 16 (dense rows of 64 / 128
    bytes: every vector path is open), 13 (a ragged last group; rows of 52 / 104 bytes) and, fp32, 260: 33 groups of 8 run as the
    compiled NG = 64, whose tile for k_pack_items_tile would take pack_items_tile_lds = 4 x 64 items x (8 x 64 + 1) words = 131,328
    bytes -- more than the 96 KB (98,304) it may -- so pack_operands takes k_pack_items there, and k_pack_items_tile at 16 and 13
    (NG = 2: 4,352 bytes).  The last run (k_pos_scores by slot) is made at 16 factors, for every pair.
    Per run: the (D, D) call against the oracle, then every pair against both, and the ledger of each strided call names the rows of
    the (D, D) call -- rows whose SPEC is not 0 wherever the table has such rows, i.e. not the check_nan rows."""
    dtype, pr = DTYPE[prec], problem(prec, factors)
    sp = Split(dev, pr["train"], pr["test"])
    placed = {side: {name: on_device(dev, pr[side], name, lay.BIG_POISON) for name in lay.LAYOUTS} for side in "AB"}
    for what, request, K, env in RUNS:
        if "RM_DEBUG_NO_POS_FLAT" in env and factors != 16:
            continue
        with switches(monkeypatch, hip, env):
            call = lambda a, b: ledger_call(hip, table, lambda: metrics_dev(hip, dev, dtype, placed["A"][a], placed["B"][b], M_USERS, N_ITEMS,
                                                                            factors, sp, K, request))
            control, rows = call(*lay.CONTROL)
            what = "%s %d factors, %s" % (prec, factors, what)
            assert rows and all(p == prec for p, _ in rows), "%s: the (D, D) call launched %s" % (what, rows)
            # (the sample seed scores its 64 items with the dump kernel, behind a pack_operands of its own: the only dump row here)
            assert any(key[2] for _, key in rows) == ("RM_DEBUG_SAMPLE_SEED" in env), "%s: the (D, D) call launched %s" % (what, rows)
            print("%s: rows %s" % (what, sorted(rows)))
            if factors <= 128:                                        # (fp32 beyond 128 factors: the table has SPEC 0 rows only)
                assert any(key[5] != 0 for _, key in rows), "%s: the (D, D) call ran check_nan rows only: %s" % (what, rows)
            assert_oracle(control, want_calc(oracle, prec, factors, K, request), dtype, what + ", (D, D) against the oracle")
            for a, b in lay.PAIRS:
                got, rows_ab = call(a, b)
                assert set(rows_ab) == set(rows), "%s, (%s, %s): launched %s, the (D, D) call %s" % (what, a, b, rows_ab, rows)
                assert_same_outputs(got, control, "%s, (%s, %s) against (D, D)" % (what, a, b))
                assert_oracle(got, want_calc(oracle, prec, factors, K, request), dtype, "%s, (%s, %s) against the oracle" % (what, a, b))


# ---- 3b. the device list entry on S ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,factors", LIST_FACTORS, ids=["%s-%d" % pf for pf in LIST_FACTORS])
def test_device_list_entry(hip, oracle, dev, prec, factors):
    """rm_recommend_dev_* at k_top = 7, NaN in every gap: ids, score bits and status against expected_lists(oracle.scores) and (D, D)"""
    dtype, pr = DTYPE[prec], problem(prec, factors)
    excl = [dev.put(x) for x in pr["train"]]
    want = want_lists(oracle, prec, factors, K_TOP)
    placed = {side: {name: on_device(dev, pr[side], name, lay.NAN_POISON) for name in lay.LAYOUTS} for side in "AB"}
    call = lambda a, b: lists_dev(hip, dev, dtype, placed["A"][a], placed["B"][b], M_USERS, N_ITEMS, factors, excl, pr["train"][1].shape[0])
    control = call(*lay.CONTROL)
    check_lists(control, want, "%s %d factors, (D, D) against the oracle" % (prec, factors))
    assert (control[2] == 0).all()
    for a, b in lay.PAIRS:
        got = call(a, b)
        check_lists(got, want, "%s %d factors, (%s, %s) against the oracle" % (prec, factors, a, b))
        check_lists(got, control, "%s %d factors, (%s, %s) against (D, D)" % (prec, factors, a, b))


# ---- 3c. the tie noise by device pointers on T ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_tie(oracle, dtype, noise):
    pr, A, B, train, test = T.problem(dtype)
    return oracle.calc(A, B, train, test, T.K, dtype=dtype, nthreads=NT, **T.KW, **(T.NOISE if noise else {}))


DEV_KW = dict(consider_cold_start=False, min_items_pool=T.K + 5, min_pos_test=0)
DEV_NOISE = dict(break_ties_with_noise=True, seed=T.NOISE["seed"])
# NoiseGeom (csrc/rm_lib.hip) for fp64 at n = 600 under RM_NOISE_BUDGET_MB=1: a user's noise row takes score_row_stride(600) = 768
# doubles and its draws 2 x 600 rounded up to whole mt19937 states of 624 = 1,248 words, 768 x 8 + 1,248 x 4 = 11,136 bytes; 2^20 / 11,136
# = 94 users per slice
NOISE_CAP_1MB = (1 << 20) // (768 * 8 + 1248 * 4)


def test_tie_noise_fp64_walks_a_in_slices(hip, oracle, dev, table, monkeypatch):
    """fp64: every user is evaluated with its noise row, in slices of what the budget holds: c.A = c0.A + b0 * c0.lda.  Under
    RM_NOISE_BUDGET_MB=1 a slice is NoiseGeom's cap = 94 users (NOISE_CAP_1MB above), so the 2,500 users are 27 slices.  Neither
    RM_HOST_TRACE (host entries only) nor rm_get_timings (the last run) reports the slices of a device call; the launch ledger does,
    indirectly: a slice is a run of the pipeline with a sweep of its own, so the sliced call launches at least three times the sweeps
    of the same call in one slice."""
    dtype = np.float64
    pr, A, B, train, test = T.problem(dtype)
    assert NOISE_CAP_1MB == 94 and T.M >= 3 * NOISE_CAP_1MB
    sp = Split(dev, train, test)
    placed = {side: {name: on_device(dev, X, name, lay.NAN_POISON) for name in lay.LAYOUTS} for side, X in (("A", A), ("B", B))}
    call = lambda a, b: ledger_call(hip, table, lambda: metrics_dev(hip, dev, dtype, placed["A"][a], placed["B"][b], T.M, T.N, T.KF, sp, T.K, ALL,
                                                                    **DEV_KW, **DEV_NOISE))
    whole, rows_whole = call(*lay.CONTROL)
    want = want_tie(oracle, dtype, True)
    assert_oracle(whole, want, dtype, "fp64 noise, (D, D) in one slice, against the oracle")
    with switches(monkeypatch, hip, {"RM_NOISE_BUDGET_MB": "1"}):
        control, rows = call(*lay.CONTROL)
        print("fp64 noise: sweeps launched in one slice %s, under RM_NOISE_BUDGET_MB=1 %s" % (rows_whole, rows))
        assert sum(rows.values()) >= 3 * sum(rows_whole.values()) > 0, (rows, rows_whole)
        assert_same_outputs(control, whole, "fp64 noise, (D, D): slices against one slice")
        for a, b in TIE_PAIRS:
            got, rows_ab = call(a, b)
            assert rows_ab == rows, "fp64 noise, (%s, %s): launched %s, the (D, D) call %s" % (a, b, rows_ab, rows)
            assert_same_outputs(got, control, "fp64 noise, (%s, %s) against (D, D)" % (a, b))
            assert_oracle(got, want, dtype, "fp64 noise, (%s, %s) against the oracle" % (a, b))


@pytest.mark.parametrize("sequential", [False, True], ids=["beside", "sequential"])
def test_tie_noise_fp32_exact_pass_gathers_rows_of_a(hip, oracle, dev, monkeypatch, sequential):
    """fp32: a first pass over everybody, then the exact pass over the flagged users alone -- beside the first sweep by default, behind
    it under RM_DEBUG_NOISE_SEQUENTIAL=1.  Either packs a subset of A's rows through slot_user (A + slot_user[slot] * lda)."""
    dtype = np.float32
    pr, A, B, train, test = T.problem(dtype)
    sp = Split(dev, train, test)
    placed = {side: {name: on_device(dev, X, name, lay.NAN_POISON) for name in lay.LAYOUTS} for side, X in (("A", A), ("B", B))}
    call = lambda a, b: metrics_dev(hip, dev, dtype, placed["A"][a], placed["B"][b], T.M, T.N, T.KF, sp, T.K, ALL, **DEV_KW, **DEV_NOISE)
    want, plain = want_tie(oracle, dtype, True), want_tie(oracle, dtype, False)
    assert any((np.nan_to_num(want[nm]) != np.nan_to_num(plain[nm])).any() for nm in want)        # the noise decides somebody's outputs
    with switches(monkeypatch, hip, {"RM_DEBUG_NOISE_SEQUENTIAL": "1"} if sequential else {}):
        control = call(*lay.CONTROL)
        assert_oracle(control, want, dtype, "fp32 noise, (D, D) against the oracle")
        for a, b in TIE_PAIRS:
            got = call(a, b)
            assert_same_outputs(got, control, "fp32 noise, (%s, %s) against (D, D)" % (a, b))
            assert_oracle(got, want, dtype, "fp32 noise, (%s, %s) against the oracle" % (a, b))


# ---- 3d. the host entries with more than one batch or shard, on T ---------------------------------------------------------------------
def traced(monkeypatch, capfd, hip, env, call):
    """call() under `env`; the batches of every user range in the host entry's own trace (RM_HOST_TRACE, one line per range on stderr)"""
    with switches(monkeypatch, hip, dict(env, RM_HOST_TRACE="1")):
        capfd.readouterr()
        got = call()
        trace = capfd.readouterr().err
    return got, sorted(int(b) for b in HOST_TRACE.findall(trace))


def host_modes(hip, monkeypatch, capfd, call, what):
    """call() as one call, in three batches, on three shards, both together, and on two shards of two batches: [(mode, result)].
    From factors a batch holds whole 1,024s of users: 2,500 users are batches of 1,024 + 1,024 + 452; three shards are ranges of 833 or
    834 users, one batch each whatever RM_BATCH_USERS says; two shards are ranges of 1,250 users = batches of 1,024 + 226, the one mode
    in which the range's first user u0 and the batch's first user b0 are both beyond 0."""
    out = [("one call", call())]
    out.append(("three batches", in_three_batches(monkeypatch, capfd, 1024, call)))
    for devices, env, batches in (([0, 0, 0], {}, [1, 1, 1]), ([0, 0, 0], {"RM_BATCH_USERS": "1024"}, [1, 1, 1]), ([0, 0], {"RM_BATCH_USERS": "1024"}, [2, 2])):
        hip.set_devices(devices)
        assert hip.get_devices() == devices
        got, traced_batches = traced(monkeypatch, capfd, hip, env, call)
        hip.set_devices([])
        mode = "%d shards%s" % (len(devices), ", RM_BATCH_USERS=1024" if env else "")
        assert traced_batches == batches, "%s, %s: batches per user range %s, expected %s" % (what, mode, traced_batches, batches)
        out.append((mode, got))
    return out


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_metric_entry_in_batches_and_shards(hip, oracle, monkeypatch, capfd, device_list, dtype, noise):
    """_binding.calc_metrics on host views (the view's base pointer and lda / ldb, not a copy), NaN in every gap: h.A + (u0 + b0) * h.lda
    and the 2-D upload for u0 > 0, for b0 > 0 and for both.  Every run equals the contiguous call in every bit."""
    pr, A, B, train, test = T.problem(dtype)
    kw = dict(T.KW, **(T.NOISE if noise else {}))
    contiguous = hip_calc(hip, A, B, train, test, T.K, dtype=dtype, **kw)
    assert_oracle(contiguous, want_tie(oracle, dtype, noise), dtype, "contiguous, one call, against the oracle")
    want = {name: True for name in hip.METRIC_ORDER}
    from oracle.oracle import NAMES
    for a, b in HOST_PAIRS:
        VA, VB = lay.place_as(A, a, lay.NAN_POISON[lay.PREC[np.dtype(dtype)]])[0], lay.place_as(B, b, lay.NAN_POISON[lay.PREC[np.dtype(dtype)]])[0]
        lda, ldb = VA.strides[0] // VA.itemsize, VB.strides[0] // VB.itemsize
        assert (lda, ldb) != (T.KF, T.KF) and not VA.flags.c_contiguous

        def call():
            outs = hip.calc_metrics(VA, lda, VB, ldb, train[0], train[1], test[0], test[1], test[2], T.K, want, True, noise, False, T.K + 5, 0, 1,
                                    kw.get("seed", 1))
            return {NAMES[name]: o for name, o in zip(hip.METRIC_ORDER, outs)}
        for mode, got in host_modes(hip, monkeypatch, capfd, call, "(%s, %s)" % (a, b)):
            assert_same_outputs(got, contiguous, "(%s, %s), %s, against the contiguous call" % (a, b, mode))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_list_entry_in_batches_and_shards(hip, oracle, monkeypatch, capfd, device_list, dtype):
    """_binding.recommend on the same host views and in the same modes: ids, score bits and status of the contiguous call"""
    pr, A, B, excl, _ = T.problem(dtype)
    contiguous = hip.recommend(A, T.KF, B, T.KF, excl[0], excl[1], K_TOP)
    check_lists(contiguous, expected_lists(oracle.scores(A, B, dtype=dtype), excl, K_TOP), "contiguous, one call, against the oracle")
    for a, b in HOST_PAIRS:
        VA, VB = lay.place_as(A, a, lay.NAN_POISON[lay.PREC[np.dtype(dtype)]])[0], lay.place_as(B, b, lay.NAN_POISON[lay.PREC[np.dtype(dtype)]])[0]
        lda, ldb = VA.strides[0] // VA.itemsize, VB.strides[0] // VB.itemsize
        call = lambda: hip.recommend(VA, lda, VB, ldb, excl[0], excl[1], K_TOP)
        for mode, got in host_modes(hip, monkeypatch, capfd, call, "lists, (%s, %s)" % (a, b)):
            check_lists(got, contiguous, "lists, (%s, %s), %s, against the contiguous call" % (a, b, mode))


# ---- 3e. special values inside a strided layout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_special_values_inside_a_strided_layout(hip, oracle, dev, table, prec):
    """Problem S at 16 factors, (RO, RO), NaN in every gap; NaN, +Inf and a large finite value at columns 0 and k - 1 of the first and
    the last rows (test_factor_layouts_cpu.py: special_problem, and on the oracle that somebody changes and not everybody).  The
    outputs equal the oracle's by the rule of test_mfma_scores_subnormal_and_special_values and the golden fixtures -- bit for bit,
    NaN for NaN -- and the ledger shows check_nan rows (SPEC 0) only, for the strided call and the (D, D) call alike, where the clean
    problem launches a row with a SPEC."""
    dtype, pr, clean = DTYPE[prec], special_problem(prec), problem(prec, SPECIAL_FACTORS)
    sp = Split(dev, pr["train"], pr["test"])
    placed = {(side, name): on_device(dev, pr[side], name, lay.NAN_POISON) for side in "AB" for name in ("D", "RO")}
    clean_ab = [on_device(dev, clean[side], "D", lay.NAN_POISON) for side in "AB"]
    for request in (TOPK8, ALL):
        call = lambda A, B: ledger_call(hip, table, lambda: metrics_dev(hip, dev, dtype, A, B, M_USERS, N_ITEMS, SPECIAL_FACTORS, sp, K_SPECIAL, request))
        _, rows_clean = call(*clean_ab)
        assert any(key[5] != 0 for _, key in rows_clean), rows_clean
        want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K_SPECIAL, metrics=request, cumulative=True, dtype=dtype, nthreads=NT)
        control, rows = call(placed["A", "D"], placed["B", "D"])
        got, rows_ro = call(placed["A", "RO"], placed["B", "RO"])
        print("special values %s %d metrics: clean %s, (D, D) %s, (RO, RO) %s" % (prec, len(request), rows_clean, rows, rows_ro))
        for r in (rows, rows_ro):
            assert r and all(p == prec and key[5] == 0 and not key[2] for p, key in r), "no check_nan row: %s" % r
        assert set(rows_ro) == set(rows)
        assert_oracle(control, want, dtype, "%s special values, (D, D) against the oracle" % prec)
        assert_same_outputs(got, control, "%s special values, (RO, RO) against (D, D)" % prec)
        assert_oracle(got, want, dtype, "%s special values, (RO, RO) against the oracle" % prec)


# ---- 3f. host batches with forced item splits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_batches_with_forced_item_splits(hip, oracle, monkeypatch, capfd, dtype):
    """T from contiguous factors, all ten metrics: three host batches (RM_BATCH_USERS=1024) whose sweeps each run over two item ranges
    and a tail level of three (RM_DEBUG_SPLITS=2,1,3) equal the single-batch, unsplit call in every bit.  The trace shows the batches,
    rm_get_timings the item ranges of the last batch."""
    pr, A, B, train, test = T.problem(dtype)
    call = lambda: hip_calc(hip, A, B, train, test, T.K, dtype=dtype, **T.KW)
    one = call()
    unsplit = hip.timings()["item_splits"]
    assert_oracle(one, want_tie(oracle, dtype, False), dtype, "one batch, unsplit, against the oracle")
    with switches(monkeypatch, hip, {"RM_DEBUG_SPLITS": "2,1,3"}):
        got = in_three_batches(monkeypatch, capfd, 1024, call)
        tm = hip.timings()
    print("item splits: unsplit call %s, under RM_DEBUG_SPLITS=2,1,3 %s" % (unsplit, tm))
    assert tm["item_splits"] == 2, "RM_DEBUG_SPLITS=2,1,3 gave %s item ranges" % tm["item_splits"]
    assert_same_outputs(got, one, "three batches with item splits against one unsplit batch")
