"""GPU: stores past the end of a workspace buffer and loads of memory nobody wrote, which a comparison of outputs cannot see.

Every device buffer of the library comes from Workspace::get (csrc/rm_lib.hip), which allocates an eighth more than it is asked for
and never shrinks a buffer: a kernel that stores a few elements too far lands in slack nobody reads, and a kernel that loads what
this call never wrote finds zeros (a fresh allocation) or the previous call's values (a reused one).  Under RM_DEBUG_WS_GUARD a buffer
lies between two red zones -- the tail zone starts at the byte count the request states -- and its payload starts poisoned (NaN words
behind ws.array<float / double>, the word 1 behind everything else).

`guarded(call)` runs a call once without and once with the mode, on a released workspace: every output must be the same in every bit
(a poisoned word that reaches an output is a load of unwritten memory), and rm_debug_ws_check must find every zone of every buffer
intact (a store past the end of a request).  The calls are the ones the other GPU files compare with the oracle, at their shapes; the
oracle comparison is theirs and is not repeated.  test_the_mechanism is the positive control: a damaged zone is reported by name, side
and offset.  The last tests put red zones around the CALLER's arrays at the device entries, which needs no mode at all."""
import functools
import os
import re

import numpy as np
import pytest

import _pairs as pairs
import _pairs_plan as pairs_plan
import _sweep_plan as sweep_plan
from _parity import hip_calc
from _requests import ALL, long_rows_problem, planted_problem
from test_hip_entry_fields import DeviceArrays, in_three_batches
from test_hip_entry_fields import KW as NOISE_KW, NOISE, K as NOISE_K, problem as noise_problem
from test_hip_recommend import iid_problem, plant_rows
from test_hip_recommend import run_host as recommend_host
from test_hip_recommend_scores import boundary_problem, run_host as recommend_scores_host
from test_hip_scores import scores_calc
from test_hip_scores_half import KINDS, half_calc, half_lists, narrow, strided_bits
from test_hip_sweep_rows import problem as sweep_problem, dump_problem, set_switches
from test_hip_sweep_rows import M_USERS as SWEEP_USERS, N_ITEMS as SWEEP_ITEMS

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPE = {"f32": F32, "f64": F64}
GUARD = "RM_DEBUG_WS_GUARD"
ZONE, RED = 256, 0xC3A55A3C                               # csrc/rm_lib.hip WS_ZONE, WS_RED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"damaged: buffer=(\w+) slot=(\d+) side=(head|tail) first=(-?\d+) last=(-?\d+) requested=(\d+) zone=(\d+)")


@pytest.fixture(scope="module")
def hip():
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device visible"
    return _binding


@pytest.fixture
def device_list(hip):
    before = hip.get_devices()
    yield
    hip.set_devices(before)


@functools.lru_cache(maxsize=None)
def buffer_ids():
    """name -> id of every workspace buffer: its place in RM_WS_BUFFERS"""
    text = open(os.path.join(ROOT, "recometrics_amd", "csrc", "rm_lib.hip")).read()
    body = text[text.index("#define RM_WS_BUFFERS(X)"):text.index("#define RM_WS_ID")]
    names = re.findall(r'^\s*X\(WS_\w+, "(\w+)"\)', body, flags=re.M)
    assert len(names) > 80 and len(set(names)) == len(names)
    return {name: i for i, name in enumerate(names)}


def arrays_of(x, path=""):
    """every array of a nested output (dicts, lists, tuples, None), with where it sits"""
    if x is None:
        return
    if isinstance(x, dict):
        for key in sorted(x):
            yield from arrays_of(x[key], "%s[%r]" % (path, key))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from arrays_of(v, "%s[%d]" % (path, i))
    else:
        yield path, np.ascontiguousarray(x)


def assert_every_bit(got, want, what):
    got, want = list(arrays_of(got)), list(arrays_of(want))
    assert [p for p, _ in got] == [p for p, _ in want], what
    for (path, g), (_, w) in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, path)
        diff = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)) // max(g.itemsize, 1)
        assert diff.size == 0, "%s: output%s differs from the run without the guard in %d elements, e.g. element %d: %r, without %r" % (
            what, path, np.unique(diff).size, diff[0], g.reshape(-1)[diff[0]], w.reshape(-1)[diff[0]])


def release(hip):
    assert hip.load().rm_release_workspace() == 0


def assert_clean(hip, what):
    damaged, checked, report = hip.ws_check()
    assert damaged == 0 and checked >= 1, "%s: %s" % (what, report)
    return checked


@pytest.fixture
def guarded(hip, monkeypatch):
    """guarded(call, what): call() without the mode, then on a released workspace with it: the same outputs in every bit, no damaged
    zone over at least one checked buffer.  stepwise=True: call(check) calls check() after each of its steps (no-op in the first run).
    Returns the number of buffers checked at the end."""
    def run(call, what, stepwise=False):
        monkeypatch.delenv(GUARD, raising=False)                        # (conftest.py: the library reads its switches again)
        plain = call(lambda: None) if stepwise else call()
        release(hip)
        monkeypatch.setenv(GUARD, "1")
        got = call(lambda: assert_clean(hip, what)) if stepwise else call()
        checked = assert_clean(hip, what)
        assert_every_bit(got, plain, what)
        print("%s: %d guarded buffers checked" % (what, checked))
        return checked
    try:
        yield run
    finally:
        monkeypatch.delenv(GUARD, raising=False)
        release(hip)


# ---- a. the mechanism ----------------------------------------------------------------------------------------------------------------
def small_call(hip):
    pr = pairs.problem(F32, 10, "iid", "none")
    return hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], 10, dtype=F32)


def damaged_zones(report):
    return sorted((name, side, int(first), int(last)) for name, _, side, first, last, _, _ in LINE.findall(report))


def test_the_mechanism(hip, monkeypatch):
    ids = buffer_ids()
    try:
        monkeypatch.delenv(GUARD, raising=False)
        release(hip)
        plain = small_call(hip)
        assert hip.ws_check()[:2] == (0, 0), "buffers allocated without the switch are not guarded"
        with pytest.raises(ValueError):
            hip.ws_poke(ids["pl"], 1, 0)                                # no guarded buffer: nothing to poke
        release(hip)
        monkeypatch.setenv(GUARD, "1")
        assert_every_bit(small_call(hip), plain, "the small call")
        damaged, checked, report = hip.ws_check()
        assert damaged == 0 and checked >= 20, report
        assert report.splitlines() == ["checked %d buffers, 0 damaged zones" % checked]
        # the positive control: one byte of pl's tail zone and one of shist's head zone
        hip.ws_poke(ids["pl"], 1, 0)
        hip.ws_poke(ids["shist"], 0, 0)
        damaged, checked2, report = hip.ws_check()
        assert damaged == 2 and checked2 == checked, report
        assert damaged_zones(report) == [("pl", "tail", 0, 0), ("shist", "head", -ZONE, -ZONE)], report
        for name, _, side, _, _, requested, zone in LINE.findall(report):
            requested, zone = int(requested), int(zone)
            cap = max(requested, 256) + max(requested, 256) // 8         # what an ordinary allocation of that request spans
            assert zone == (ZONE if side == "head" else (cap + 3) // 4 * 4 + ZONE - requested), report
            assert side == "head" or zone >= ZONE + requested // 8, report
        # a switch flipped in mid-process: the guarded buffers stay guarded, are still checked, and are freed as what they are
        monkeypatch.delenv(GUARD)
        assert hip.ws_check()[0] == 2
        release(hip)
        assert hip.ws_check()[:2] == (0, 0)
        # the last byte of a tail zone, and both ends of a head zone
        monkeypatch.setenv(GUARD, "1")
        small_call(hip)
        hip.ws_poke(ids["merged"], 1, -1)
        hip.ws_poke(ids["flags"], 0, -1)
        hip.ws_poke(ids["flags"], 0, 3)
        damaged, _, report = hip.ws_check()
        found = {(name, side): (int(first), int(last), int(zone)) for name, _, side, first, last, _, zone in LINE.findall(report)}
        assert damaged == 2 and set(found) == {("merged", "tail"), ("flags", "head")}, report
        assert found[("merged", "tail")][:2] == (found[("merged", "tail")][2] - 1,) * 2 and found[("flags", "head")][:2] == (3 - ZONE, -1), report
        with pytest.raises(ValueError):
            hip.ws_poke(ids["flags"], 0, ZONE)                          # outside the zone: refused, nothing is written
        with pytest.raises(ValueError):
            hip.ws_poke(len(ids), 1, 0)
        release(hip)
        assert hip.ws_check()[:2] == (0, 0)
        assert_every_bit(small_call(hip), plain, "a fresh guarded workspace after the damaged one")
        assert_clean(hip, "after the release")
    finally:
        monkeypatch.delenv(GUARD, raising=False)
        release(hip)


def test_damage_in_what_a_larger_request_takes_over_is_kept(hip, monkeypatch):
    """a request that is larger than every one before and fits the buffer's slack gets the same buffer, as without the mode: the
    payload grows into the tail zone.  Damage in the part taken over is found then and stays in the report; the rest is no damage."""
    pr = pairs.problem(F32, 33, "iid", "none")
    call = lambda K: hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, cumulative=True, dtype=F32)
    try:
        release(hip)
        monkeypatch.setenv(GUARD, "1")
        call(32)
        assert_clean(hip, "K = 32")
        call(33)                                                        # (the metric block and the lists: 3 % larger, inside an eighth of slack)
        assert_clean(hip, "K = 32, then K = 33 in the same buffers")
        release(hip)
        call(32)
        hip.ws_poke(buffer_ids()["o_block"], 1, 5)
        damaged, _, report = hip.ws_check()
        assert damaged == 1 and damaged_zones(report) == [("o_block", "tail", 5, 5)], report
        before = int(LINE.search(report).group(6))
        call(33)
        damaged, _, report = hip.ws_check()
        assert damaged == 1 and damaged_zones(report) == [("o_block", "tail", 5, 5)], report
        assert int(LINE.search(report).group(6)) == before, "the report names the request the damaged byte lay behind: " + report
    finally:
        monkeypatch.delenv(GUARD, raising=False)
        release(hip)


# ---- b. every case of the pairwise plan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pairs_plan.CASES, ids=[pairs_plan.case_id(c) for c in pairs_plan.CASES])
def test_pairwise_plan(hip, oracle, guarded, case, monkeypatch, device_list):
    pr, K, dtype, kw = pairs.problem_of(case), case.K, pairs.DTYPE[case.dtype], pairs_plan.call_kw(case)
    for name in ("RM_BATCH_USERS", "RM_DEBUG_SPLITS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in pairs_plan.env_of(case).items():
        monkeypatch.setenv(name, value)
    hip.set_devices(pairs_plan.DEVICES[case.devices])

    def call():
        if case.entry == "scores":
            opts = {k: v for k, v in kw.items() if k not in ("noise", "seed")}
            return scores_calc(hip, pairs.scores(oracle, pr, dtype), pr["train"], pr["test"], K, dtype=dtype, **opts)
        return hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, dtype=dtype, **kw)
    guarded(call, pairs_plan.case_id(case))


# ---- c. every sweep unit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,unit", sweep_plan.unit_ids(), ids=["%s-%s" % pu for pu in sweep_plan.unit_ids()])
def test_sweep_units(hip, guarded, prec, unit, monkeypatch):
    from scipy.sparse import csr_array
    from recometrics_amd import recommend_topk
    visits = sweep_plan.visits_of(prec, unit)
    assert visits

    def call():
        out = []
        for v in visits:
            set_switches(monkeypatch, v.env)                            # (the guard is none of the plan's switches: it stays as it is)
            if v.kind == "dump":
                out.append(hip.debug_scores(*dump_problem(v.prec, v.factors)))
                continue
            pr = sweep_problem(v.prec, v.factors)
            out.append(hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], v.K, metrics=v.request, cumulative=True, dtype=DTYPE[v.prec]))
            trp, tri = pr["train"]
            if v.request == sweep_plan.ALL:
                out.append(hip.rank(pr["A"], pr["B"], trp, tri, pr["test"][0], pr["test"][1], v.K))
            else:
                X = csr_array((np.ones(tri.shape[0], np.float32), tri, trp), shape=(SWEEP_USERS, SWEEP_ITEMS))
                out.append(list(recommend_topk(pr["A"], pr["B"], k=v.K, X_train=X)))
        return out
    guarded(call, "%s %s" % (prec, unit))


# ---- d. long test rows -----------------------------------------------------------------------------------------------------------------
LONG_ENVS = [{}, {"RM_STREAM_BUDGET_MB": "0"}, {"RM_STREAM_BUDGET_MB": "1"}, {"RM_DEBUG_RANK_GENERIC": "1"}]


@pytest.mark.parametrize("env", LONG_ENVS, ids=["budget_unset", "budget_0", "budget_1", "rank_generic"])
@pytest.mark.parametrize("K", [10, 100, 256])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_long_test_rows(hip, guarded, monkeypatch, dtype, K, env):
    """rows of 1 to 4,000 test items: k_rank_streamed in all of its table depths and its global-memory fall-back, k_auc_streamed,
    k_top_values, k_select_topk (K = 256: score rows for everybody), and with a budget of 0 the rows in chunks"""
    pr = long_rows_problem(dtype)
    for name in ("RM_STREAM_BUDGET_MB", "RM_DEBUG_RANK_GENERIC"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    guarded(lambda: [hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], K, metrics=ALL, cumulative=cum, dtype=dtype) for cum in (False, True)],
            "long rows %s K=%d %s" % (np.dtype(dtype).name, K, env))


# ---- e. tie noise ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"RM_DEBUG_NOISE_SEQUENTIAL": "1"}, {"RM_DEBUG_NOISE_PER_BATCH": "1"}], ids=["default", "sequential", "per_batch"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_tie_noise(hip, guarded, monkeypatch, capfd, dtype, env):
    """2,500 users in one batch and in three: fp32's first pass, flags, exact pass, gather and scatter; fp64's exact noise rows"""
    _, A, B, train, test = noise_problem(dtype)
    for name in ("RM_DEBUG_NOISE_SEQUENTIAL", "RM_DEBUG_NOISE_PER_BATCH"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    one = lambda: hip_calc(hip, A, B, train, test, NOISE_K, dtype=dtype, **NOISE_KW, **NOISE)
    guarded(lambda: [one(), in_three_batches(monkeypatch, capfd, 1024, one)], "tie noise %s %s" % (np.dtype(dtype).name, env))


# ---- f. lists --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 100, 300, 1500])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lists_from_factors(hip, guarded, dtype, K):
    """tests/test_hip_recommend.py's users with few candidates, at a K of every list scheme"""
    m, n = 80, 2000
    A, B, excl = iid_problem(m, n, 64, dtype, 31)
    excl = plant_rows(excl, n, {0: n, 3: 0, 5: 1, 6: 3, 40: K - 1, 41: K, 42: K + 1, 77: 1, 78: 3, 79: K - 1})
    guarded(lambda: [recommend_host(hip, A, B, excl, K), recommend_host(hip, A, B, None, K, scores=False)], "recommend K=%d" % K)


@pytest.mark.parametrize("K", [10, 1024, 1025])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lists_from_scores(hip, guarded, dtype, K):
    S, excl = boundary_problem(dtype)
    guarded(lambda: [recommend_scores_host(hip, S, excl, K), recommend_scores_host(hip, S, None, K, scores=False)], "recommend_scores K=%d" % K)


@functools.lru_cache(maxsize=None)
def half_rows(kind, m=48, n=6000):
    """16-bit scores, rows n + 3 apart and the first one 2 bytes past a 16-byte boundary"""
    return strided_bits(narrow(np.random.default_rng(33).standard_normal((m, n)), kind), n + 3, 1)


@pytest.mark.parametrize("K", [10, 1024, 1025])
@pytest.mark.parametrize("kind", KINDS)
def test_lists_from_16_bit_scores(hip, guarded, kind, K):
    excl = boundary_problem(F32)[1]
    guarded(lambda: half_lists(hip, half_rows(kind), kind, excl, K), "recommend_scores_%s K=%d" % (kind, K))


# ---- g. other entries ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_scores(oracle, dtype, K):
    pr = planted_problem(700, 4099, 16, dtype, 7, K)
    return pr, oracle.scores(pr["A"], pr["B"], dtype=dtype)


@pytest.mark.parametrize("K", [10, 300, 4099])
@pytest.mark.parametrize("kind", ["f32", "f64", "f16", "bf16"])
def test_metrics_from_scores(hip, oracle, guarded, kind, K):
    """n = 4,099 and 700 users with the users planted for this K, rows n + 3 apart"""
    dtype = DTYPE.get(kind, F32)
    pr, S = planted_scores(oracle, dtype, K)
    if kind in KINDS:
        view = strided_bits(narrow(S, kind), S.shape[1] + 3, 1)
        call = lambda: [half_calc(hip, view, kind, pr["train"], pr["test"], K, cumulative=cum) for cum in (False, True)]
    else:
        call = lambda: [scores_calc(hip, S, pr["train"], pr["test"], K, cumulative=cum, pad=3, dtype=dtype) for cum in (False, True)]
    guarded(call, "metrics from %s scores K=%d" % (kind, K))


@pytest.mark.parametrize("noise", [False, True], ids=["noise_off", "noise_on"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_rank(hip, guarded, dtype, noise):
    pr = pairs.problem(dtype, 10, "iid", "third")
    (trp, tri), (tep, tei) = pr["train"], pr["test"][:2]
    guarded(lambda: hip.rank(pr["A"], pr["B"], trp, tri, tep, tei, 10, break_ties_with_noise=noise, seed=5), "rank")


# ---- h. kept split and warm bounds -----------------------------------------------------------------------------------------------------
KEPT = [("f32", {}), ("f32", {"RM_DEBUG_NO_TRAIN_BITS": "1"}), ("f64", {"RM_DEBUG_LANE_MIN_K": "1000"}),
        ("f64", {"RM_DEBUG_LANE_MIN_K": "1000", "RM_DEBUG_NO_TRAIN_BITS": "1"})]


@pytest.mark.parametrize("models", [(100, 101, 102), (100, 100, 100)], ids=["three_models", "one_model_three_times"])
@pytest.mark.parametrize("prec,env", KEPT, ids=["%s-%s" % (p, "-".join(sorted(e)) or "defaults") for p, e in KEPT])
def test_three_calls_on_a_kept_split(hip, guarded, monkeypatch, prec, env, models):
    """the device entry on one split, no release between the calls and a check after each: the second and third call run in the
    buffers the first one sized, on the plan it kept, and seed their bounds from the lists the call before left (k_hint_bounds)"""
    from recometrics_amd.synth import make_factors
    from _split_cache_child import split_arrays, M, N, KF
    dtype, K = DTYPE[prec], 10
    for name in ("RM_DEBUG_NO_TRAIN_BITS", "RM_DEBUG_LANE_MIN_K"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    arrays = split_arrays(dtype)
    dev = DeviceArrays(hip)
    seen = []
    try:
        d = [dev.put(a) for a in arrays]
        factors = {seed: [dev.put(x) for x in make_factors(M, N, KF, dtype, seed=seed)] for seed in set(models)}
        outs = [dev.put(np.full(M, -7, dtype)) for _ in range(10)]

        def call(check):
            hip.reload_switches()                                       # (voids what a context kept of an earlier split at these addresses)
            got, reused, hinted = [], [], []
            for seed in models:
                A, B = factors[seed]
                hip.calc_metrics_device(dtype, A, KF, B, KF, M, N, KF, d[0], d[1], arrays[1].shape[0], d[2], d[3], d[4], arrays[3].shape[0], K, outs)
                got.append([dev.get(o, (M,), dtype) for o in outs])
                reused.append(hip.timings().get("split_reused"))
                hinted.append(hip.hinted_users())
                check()
            seen.append((reused, hinted))
            return got
        guarded(call, "kept split %s %s" % (prec, env), stepwise=True)
    finally:
        dev.free()
    # without the guard and with it, the same path: the plan reused twice, bounds from the first call's lists in the second (and, where
    # the model stays, in the third: after another model's lists the library may stand down for a call)
    assert len(seen) == 2 and seen[0] == seen[1], seen
    reused, hinted = seen[1]
    assert reused == [0, 1, 1] and hinted[0] == 0 and hinted[1] > 0 and (hinted[2] > 0 or len(set(models)) > 1), seen


# ---- i. the caller's own arrays at the device entries ----------------------------------------------------------------------------------
class Slab:
    """one device allocation that holds every array of a call: each one starts on a 256-byte boundary with ZONE bytes of the red word
    in front of it, the red word goes on from its last byte to the next array's front zone, and ZONE bytes close the slab"""
    def __init__(self):
        self.parts, self.size = {}, ZONE

    def add(self, name, array):
        array = np.ascontiguousarray(array)
        self.parts[name] = (self.size, array)
        self.size = (self.size + array.nbytes + 255) // 256 * 256 + ZONE
        return self

    def image(self):
        img = np.tile(np.frombuffer(np.uint32(RED).tobytes(), np.uint8), self.size // 4)
        for at, a in self.parts.values():
            img[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
        return img

    def upload(self, dev):
        self.dev, self.before = dev, self.image()
        self.base = dev.put(self.before)
        return self

    def ptr(self, name):
        return self.base + self.parts[name][0]

    def collect(self, outputs, what):
        """the outputs' arrays after the call; every other byte of the slab -- red zones and inputs -- is what was uploaded"""
        after = self.dev.get(self.base, (self.size,), np.uint8)
        got, untouched = {}, np.ones(self.size, bool)
        for name in outputs:
            at, a = self.parts[name]
            got[name] = after[at:at + a.nbytes].view(a.dtype).reshape(a.shape).copy()
            untouched[at:at + a.nbytes] = False
        changed = np.flatnonzero(untouched & (after != self.before))
        if changed.size:
            at = int(changed[0])
            owner = max((p for p in self.parts.items() if p[1][0] - ZONE <= at), key=lambda p: p[1][0])
            raise AssertionError("%s: %d bytes outside the outputs changed, the first %d bytes from the start of %r (%d bytes long)" % (
                what, changed.size, at - owner[1][0], owner[0], owner[1][1].nbytes))
        return got


def entry_problem(dtype):
    pr = pairs.problem(dtype, 10, "iid", "third")
    A, B = np.ascontiguousarray(pr["A"], dtype), np.ascontiguousarray(pr["B"], dtype)
    train = [np.ascontiguousarray(x, np.int32) for x in pr["train"]]
    test = [np.ascontiguousarray(x, np.int32) for x in pr["test"][:2]] + [np.ascontiguousarray(pr["test"][2], dtype)]
    return A, B, train, test


# (the 16-bit entries are fp32 entries: every array but S is the _f32 entry's)
DEVICE_ENTRIES = [(F32, "factors"), (F32, "scores"), (F32, "f16"), (F32, "bf16"), (F64, "factors"), (F64, "scores")]


@pytest.fixture()
def dev(hip):
    d = DeviceArrays(hip)
    yield d
    d.free()


@pytest.mark.parametrize("request_", [ALL, ("p", "r", "ap", "ndcg", "hit", "rr", "roc")], ids=["all", "without_tp_tap_pr"])
@pytest.mark.parametrize("dtype,source", DEVICE_ENTRIES, ids=["%s-%s" % (np.dtype(d).name, s) for d, s in DEVICE_ENTRIES])
def test_metric_device_entries_write_their_outputs_only(hip, dev, dtype, source, request_):
    from oracle.oracle import NAMES
    A, B, train, test = entry_problem(dtype)
    (m, kf), n, K = A.shape, B.shape[0], 10
    S = hip.debug_scores(A, B)
    slab = Slab().add("train_p", train[0]).add("train_i", train[1]).add("test_p", test[0]).add("test_i", test[1]).add("test_v", test[2])
    if source == "factors":
        slab.add("A", A).add("B", B)
    else:
        slab.add("S", narrow(S, source) if source in KINDS else S)
    wanted = [name for name in hip.METRIC_ORDER if name in request_]
    for name in wanted:
        slab.add(name, np.full((m,) if name in ("roc", "pr") else (m, K), 7, dtype))
    slab.upload(dev)
    outs = [slab.ptr(name) if name in wanted else 0 for name in hip.METRIC_ORDER]
    split = (slab.ptr("train_p"), slab.ptr("train_i"), train[1].shape[0], slab.ptr("test_p"), slab.ptr("test_i"), slab.ptr("test_v"), test[1].shape[0])
    if source == "factors":
        hip.calc_metrics_device(dtype, slab.ptr("A"), kf, slab.ptr("B"), kf, m, n, kf, *split, K, outs, cumulative=True)
        want = hip_calc(hip, A, B, train, test, K, metrics=request_, cumulative=True, dtype=dtype)
    elif source == "scores":
        hip.calc_metrics_scores_device(dtype, slab.ptr("S"), n, m, n, *split, K, outs, cumulative=True)
        want = scores_calc(hip, S, train, test, K, metrics=request_, cumulative=True, dtype=dtype)
    else:
        hip.calc_metrics_scores_half_device(source, slab.ptr("S"), n, m, n, *split, K, outs, cumulative=True)
        want = half_calc(hip, narrow(S, source), source, train, test, K, metrics=request_, cumulative=True)
    got = slab.collect(wanted, "%s %s" % (source, np.dtype(dtype).name))
    assert_every_bit({NAMES[name]: got[name] for name in wanted}, want, "the device entry against the host entry")


@pytest.mark.parametrize("dtype,source", DEVICE_ENTRIES, ids=["%s-%s" % (np.dtype(d).name, s) for d, s in DEVICE_ENTRIES])
def test_list_device_entries_write_their_outputs_only(hip, dev, dtype, source):
    A, B, excl, _ = entry_problem(dtype)
    (m, kf), n, K = A.shape, B.shape[0], 10
    S = hip.debug_scores(A, B)
    slab = Slab().add("excl_p", excl[0]).add("excl_i", excl[1])
    if source == "factors":
        slab.add("A", A).add("B", B)
    else:
        slab.add("S", narrow(S, source) if source in KINDS else S)
    slab.add("idx", np.full((m, K), 77, np.int32)).add("score", np.full((m, K), 7, dtype)).add("status", np.full(m, 77, np.int32)).upload(dev)
    tail = (slab.ptr("excl_p"), slab.ptr("excl_i"), excl[1].shape[0], K, slab.ptr("idx"), slab.ptr("score"), slab.ptr("status"))
    if source == "factors":
        hip.recommend_device(dtype, slab.ptr("A"), kf, slab.ptr("B"), kf, m, n, kf, *tail)
        want = recommend_host(hip, A, B, excl, K)
    elif source == "scores":
        hip.recommend_scores_device(dtype, slab.ptr("S"), n, m, n, *tail)
        want = recommend_scores_host(hip, S, excl, K)
    else:
        hip.recommend_scores_half_device(source, slab.ptr("S"), n, m, n, *tail)
        want = half_lists(hip, narrow(S, source), source, excl, K)
    got = slab.collect(["idx", "score", "status"], "%s %s" % (source, np.dtype(dtype).name))
    assert_every_bit([got["idx"], got["score"], got["status"]], list(want), "the device entry against the host entry")
