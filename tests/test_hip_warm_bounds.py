"""GPU: a call on the split the context kept seeds its top-K bounds from the lists the call before it left (k_hint_bounds).

The device-pointer entry with torch tensors as memory owners, one process per configuration (switches are read at load):
tests/_warm_bounds_child.py plays the scenarios and compares every output array of every call, bit for bit, with the same call under
RM_DEBUG_NO_WARM_BOUNDS=1 on freshly allocated arrays; here the last call of every scenario also goes against the oracle (bitwise,
ROC-AUC by assert_roc: _check_against_oracle's rules), and the number of users that got a bound (rm_get_timings out[11]) against
tests/_warm_bounds.py's restatement of the kernel's rejection rules.

300 users x 700 items, make_interactions with a mean of 120 and half of every row held out: table users of every depth, streamed users,
users without a train row or a test row, and one user with ten candidates.  The bounds are for the calls whose lists are the
replace-the-minimum ones: fp32 below k_metrics = 20 at these factor counts, fp64 only where RM_DEBUG_LANE_MIN_K keeps the lane buffers
away (as it does here for the fp64 configurations that expect bounds); a lane-buffer call must report none and compute the same."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _parity import NT
from _util import assert_roc, assert_same_bits
from test_hip_parity import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LISTS = {"RM_DEBUG_LANE_MIN_K": "1000"}
NO_BITS = {"RM_DEBUG_NO_TRAIN_BITS": "1"}


def _cfg(prec="f32", K=10, kf=16, layout="D", full=False, hints=True, env=None):
    return dict(prec=prec, K=K, kf=kf, layout=layout, full=full, hints=hints, env=env or {})


CONFIGS = {
    "f32-dense_rows": _cfg(full=True),
    "f32-no_train_bits": _cfg(full=True, env=NO_BITS),
    "f64-dense_rows": _cfg("f64", full=True, env=LISTS),
    "f64-no_train_bits": _cfg("f64", full=True, env=dict(LISTS, **NO_BITS)),
    "f64-lane_buffers": _cfg("f64", hints=False),
    "f32-K1": _cfg(K=1),
    "f32-K5": _cfg(K=5),
    "f32-K20-lane_buffers": _cfg(K=20, hints=False),
    "f32-K20-lists": _cfg(K=20, env=LISTS),
    "f32-50_factors": _cfg(kf=50),
    "f32-stride_and_offset": _cfg(layout="RO"),
    "f64-stride_and_offset": _cfg("f64", layout="RO", env=LISTS),
}
FULL = [name for name, c in CONFIGS.items() if c["full"]]


@functools.lru_cache(maxsize=None)
def _played(name):
    cfg = CONFIGS[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RM_")}
    env.update(cfg["env"])
    spec = json.dumps({k: v for k, v in cfg.items() if k != "env"})
    res = subprocess.run([sys.executable, os.path.join(HERE, "_warm_bounds_child.py"), spec], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def _wanted(oracle, prec, K, kf, model):
    """the oracle's metrics of one model on the child's split: computed once, shared, never changed"""
    from _warm_bounds_child import model as factors, split_arrays
    dtype = np.float32 if prec == "f32" else np.float64
    A, B = factors(model, kf, dtype)
    trp, tri, tep, tei, tev = split_arrays(dtype)
    return oracle.calc(A, B, (trp, tri), (tep, tei, tev), K, cumulative=False, dtype=dtype, nthreads=NT)


def _against_oracle(hip, oracle, name, model, outputs, what):
    from oracle.oracle import NAMES
    cfg = CONFIGS[name]
    dtype = np.float32 if cfg["prec"] == "f32" else np.float64
    want = _wanted(oracle, cfg["prec"], cfg["K"], cfg["kf"], model)
    for metric, values in zip(hip.METRIC_ORDER, outputs):
        mine = np.asarray(values, dtype=np.float64).astype(dtype)          # (floats survive JSON exactly)
        if NAMES[metric] == "ROC_AUC":
            assert_roc(mine, want[NAMES[metric]], dtype, "%s, %s" % (what, metric))
        else:
            assert_same_bits(mine, want[NAMES[metric]], "%s, %s (bitwise)" % (what, metric))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_same_model_twice_then_a_third_time(hip, oracle, name):
    """no bound on the first call; on the second and third exactly the users whose K ids of the call before are all >= 0 (distinct,
    no train items: they are a list) and who are evaluated for ranks in one slot -- computed on the CPU from the base model's scores"""
    got = _played(name)
    E = got["expect"]
    pop = got["population"]
    assert pop["evaluated"] < pop["users"], "users that are not evaluated (no test row, no train row) take part"
    if CONFIGS[name]["hints"]:
        assert 0 < E <= pop["evaluated"], (E, pop)
    assert got["off"]["hinted"] == [0, 0, 0], got["off"]
    same = got["same"]
    assert same["reused"] == [0, 1, 1] and same["equal"] == [True, True, True], same
    assert same["hinted"] == [0, E, E], (same["hinted"], E)
    _against_oracle(hip, oracle, name, "base", same["outputs"], "third call on the same model")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_another_model_on_the_kept_lists(hip, oracle, name):
    """factors of another seed, -A (the previous best become the worst), A scaled by 1e-3, scores ascending in the item id, runs of
    exact ties (at the K-th place too), spikes, and two clusters (all previous top-K scores equal): the bound is valid or absent and the
    bits are equal.  The number of users with a bound does not depend on the model: its scores are finite."""
    got = _played(name)
    E = got["expect"]
    assert set(got["drift"]) == (set(("seed", "neg", "scaled", "ascending", "runs", "spikes", "clusters")) if CONFIGS[name]["full"] else {"neg"})
    for model, d in got["drift"].items():
        assert d["reused"] == [0, 1, 1] and d["equal"] == [True, True, True], (model, d)
        assert d["hinted"][:2] == [0, E], (model, d["hinted"], E)
        # (the third call runs on the lists of the drifted model, unless that model's bounds raised too few words and the kernel stands
        # down for a pass -- test_standing_down; full lists for the tie-free models, fewer where a user was invalid)
        assert d["hinted"][2] in (0, E) if model in ("seed", "neg", "scaled") else 0 <= d["hinted"][2] <= E, (model, d["hinted"], E)
        if model == "scaled":
            assert d["hinted"][2] == E, "the same ranking at a thousandth of the scale: every bound is the final K-th best"
        _against_oracle(hip, oracle, name, model, d["outputs"], "%s on the lists of the base model" % model)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_standing_down(name):
    """base, -A, base, base, base, then -A five times, base.  A bound raises a user's word when it lies above the K-th best of the user's own
    test items; the base model's previous best items are -A's worst, so the second call's bounds raise next to nothing (fewer than half
    of them: the test rows hold 60 items on average, K of them bound better than the ten worst scores) and the third call runs
    without the kernel.  The fourth tries again on the lists of the third -- the same model: every bound is the final K-th best, the
    back-off is over and the fifth runs with bounds.  From the sixth on the model alternates no more but stays useless relative to the lists
    it is given (each -A call's lists are its own, so a -A call behind a -A call raises everything): launched, skipped or launched is
    decided by the back-off alone, and the bits are equal throughout."""
    got = _played(name)
    E = got["expect"]
    s = got["stand_down"]
    assert s["equal"] == [True] * 11, s
    assert s["reused"] == [0] + [1] * 10, s
    if not CONFIGS[name]["hints"]:
        assert s["hinted"] == [0] * 11, s
        return
    assert s["hinted"][:5] == [0, E, 0, E, E], (s["hinted"], E)
    # call 6 (-A on base's lists) raises little: call 7 stands down; call 8 (-A on -A's lists) raises everything; 9, 10 run with bounds;
    # call 11 (base on -A's lists) is launched and raises little
    assert s["hinted"][5:] == [E, 0, E, E, E, E], (s["hinted"], E)
    # base and -A in turn, twelve calls: every launch finds the other model's lists, and the pauses behind it are 1, 2, 4 passes long
    b = got["back_off"]
    assert b["equal"] == [True] * 12, b
    assert b["hinted"] == [0, E, 0, E, 0, 0, E, 0, 0, 0, 0, E], (b["hinted"], E)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_poisoned_advice(hip, oracle, name):
    """ids overwritten through rm_debug_set_list_ids: duplicates, a train item, -1, n, the list of another user (which holds a train item
    of this one) take the bound away from exactly the users concerned; K of the user's own test items are legal advice.  Equal bits
    always."""
    got = _played(name)
    E = got["expect"]
    cfg = CONFIGS[name]
    assert set(got["poison"]) == (set(("duplicates", "train_item", "minus_one", "index_n", "other_user", "test_items")) if cfg["full"] else {"duplicates", "test_items"})
    for kind, p in got["poison"].items():
        assert p["equal"] == [True, True], (kind, p)
        if cfg["hints"]:
            assert p["users"] > 0 or (kind == "duplicates" and cfg["K"] == 1) or (kind == "test_items" and cfg["K"] > 10), (kind, p)
            drop = 0 if kind == "test_items" else p["users"]
            assert p["restated"] == E - drop, (kind, p, E)
        assert p["hinted"] == [0, p["restated"]], (kind, p)
        _against_oracle(hip, oracle, name, "base", p["outputs"], "poisoned advice: %s" % kind)


@pytest.mark.parametrize("name", FULL)
def test_what_voids_the_lists(hip, oracle, name):
    """a changed test item between two calls, another k_metrics, another request, a released workspace, a tie-noise call in between:
    the next plain call gets no bound, and the one after it does.

    The tie-noise call: its first pass goes through the context's pipeline like every call, is not a plain pass, and so voids what the
    context keeps of the split -- the lists' record is part of that record and goes with it (its exact passes run on a context of their
    own and would not have touched `merged`; the record does not try to survive on that)."""
    got = _played(name)
    E = got["expect"]
    v = got["void"]
    c = v["changed_test_item"]
    assert c["reused"] == [0, 0, 1] and c["hinted"] == [0, 0, E] and c["equal"] == [True] * 3, c
    k = v["other_K"]
    assert k["reused"] == [0, 0, 0, 1] and k["hinted"] == [0, 0, 0, E] and k["equal"] == [True] * 4, k
    r = v["other_request"]
    assert r["reused"] == [0, 0, 0] and r["hinted"] == [0, 0, 0] and r["equal"] == [True] * 3, r
    w = v["release"]
    assert w["reused"] == [0, 0, 1] and w["hinted"] == [0, 0, E] and w["equal"] == [True] * 3, w
    _against_oracle(hip, oracle, name, "base", w["outputs"], "second call behind a released workspace")
    t = v["tie_noise_between"]
    assert t["reused"] == [0, -1, 0, 1] and t["hinted"] == [0, 0, 0, E] and t["equal"] == [True] * 4, t
    assert v["hook_refuses"] == [True, True], v["hook_refuses"]
