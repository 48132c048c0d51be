"""Child process of tests/test_hip_warm_bounds.py: torch owns the device memory (loaded before the library), the calls go through
_binding.calc_metrics_device.  Usage: python _warm_bounds_child.py '<json spec>' -- prints one JSON line, scenario -> findings.
Spec: prec f32|f64, K, kf (factors), layout (a name of tests/_layouts.py for A and for B), full (every scenario, or the core only).

Phase 0 scores the base model once (rm_debug_scores_*: the sweep's scores) and restates the lists a call on it leaves (_warm_bounds).
Phase 1 runs every call the scenarios make with RM_DEBUG_NO_WARM_BOUNDS=1, each on freshly allocated arrays: the yardstick.
Phase 2 switches the warm bounds on and plays the scenarios; every output array of every call must equal its yardstick bit for bit,
and the number of users that got a bound (rm_get_timings out[11]) must be the number _warm_bounds.hintable gives."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from recometrics_amd import _binding as hip          # noqa: E402
from recometrics_amd.synth import make_factors, make_interactions, make_structured          # noqa: E402
from _layouts import LAYOUTS, NAN_POISON, place          # noqa: E402
from _util import same_bits          # noqa: E402
import _warm_bounds as wb          # noqa: E402

M, N, MEAN = 300, 700, 120
ALL = tuple(range(10))
SPEC = json.loads(sys.argv[1]) if __name__ == "__main__" else {"prec": "f32", "K": 10, "kf": 16, "layout": "D", "full": False}
PREC, K0, KF, LAYOUT, FULL = SPEC["prec"], SPEC["K"], SPEC["kf"], SPEC["layout"], SPEC["full"]
DT = {"f32": np.float32, "f64": np.float64}[PREC]
DRIFTS = ("seed", "neg", "scaled", "ascending", "runs", "spikes", "clusters")

dev = torch.device("cuda", 0)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def split_arrays(dtype=DT):
    """the split of tests/_split_cache_child.py: half of every row held out (streamed users next to table users of every depth), two
    users without a train row, two without a test row; and one user with ten candidates (its train row: all items but ten), who
    is evaluated up to k_metrics = 10 -- every candidate is then on its list -- and not at all beyond"""
    trp, tri, tep, tei, tev = make_interactions(M, N, MEAN, dtype, seed=5, test_fraction=0.5)

    def with_rows(p, arrays, rows):
        """rows: user -> the new index row (values: ones)"""
        chunks = [[a[p[u]:p[u + 1]] for a in arrays] for u in range(M)]
        for u, idx in rows.items():
            chunks[u] = [np.asarray(idx, arrays[0].dtype)] + [np.ones(len(idx), a.dtype) for a in arrays[1:]]
        q = np.zeros_like(p)
        np.cumsum([c[0].shape[0] for c in chunks], out=q[1:])
        return [q] + [np.concatenate([c[i] for c in chunks]) for i in range(len(arrays))]
    few = 123
    keep = np.union1d(tei[tep[few]:tep[few + 1]][:4], np.arange(5, N, 87))[:10]
    trp, tri = with_rows(trp, [tri], {17: [], 40: [], few: np.setdiff1d(np.arange(N), keep)})
    tep, tei, tev = with_rows(tep, [tei, tev], {40: [], 77: [], few: keep[:3]})
    return [trp, tri, tep, tei, tev]


BASE = split_arrays()


def model(name, kf=KF, dtype=DT):
    A, B = make_factors(M, N, kf, dtype, seed=100)
    if name == "base":
        return A, B
    if name == "seed":
        return make_factors(M, N, kf, dtype, seed=101)
    if name == "neg":                      # the previous best become the worst
        return -A, B
    if name == "scaled":
        return (A * dtype(1e-3)).astype(dtype), B
    kind, variant = {"ascending": ("ascending", "spikes"), "runs": ("runs", "spikes"), "spikes": ("outliers", "spikes"),
                     "clusters": ("outliers", "clusters")}[name]
    pr = make_structured(kind, M, N, kf, dtype, mean_c=10, seed=9, variant=variant)
    return pr["A"], pr["B"]


class Split:
    def __init__(self, arrays):
        self.np = [a.copy() for a in arrays]
        self.d = [t(a) for a in self.np]

    def poke(self, which, at, value):
        self.np[which][at] = value
        self.d[which][at] = value.item() if hasattr(value, "item") else value
        torch.cuda.synchronize()


def on_device(X):
    """the matrix in the layout of the spec: (owner tensor, address of X[0, 0], leading dimension)"""
    pad, off = LAYOUTS[LAYOUT][PREC]
    V, raw, at = place(X, pad, off, NAN_POISON[PREC])
    owner = t(raw)
    return owner, owner.data_ptr() + at * X.itemsize, X.shape[1] + pad


def call(sp, name, K=K0, metrics=ALL, noise=False):
    """one metric call; returns (outputs, split_reused, users with a warm bound)"""
    A, B = model(name)
    oa, pa, lda = on_device(A)
    ob, pb, ldb = on_device(B)
    tt = torch.float32 if DT == np.float32 else torch.float64
    outs = [torch.full((M,), -7.0, dtype=tt, device=dev) if i in metrics else None for i in range(10)]
    hip.calc_metrics_device(DT, pa, lda, pb, ldb, M, N, KF, sp.d[0].data_ptr(), sp.d[1].data_ptr(), sp.np[1].shape[0],
                            sp.d[2].data_ptr(), sp.d[3].data_ptr(), sp.d[4].data_ptr(), sp.np[3].shape[0], K,
                            [o.data_ptr() if o is not None else 0 for o in outs], break_ties_with_noise=noise, seed=3)
    torch.cuda.synchronize()
    return [o.cpu().numpy() if o is not None else None for o in outs], int(hip.timings().get("split_reused")), hip.hinted_users()


def equal(got, want):
    return all((g is None and w is None) or bool(same_bits(g, w).all()) for g, w in zip(got[0], want[0]))


def first_use(arrays=BASE):
    """a split nothing is kept of (a reload of the switches voids what the contexts keep)"""
    hip.reload_switches()
    return Split(arrays)


def floats(outs):
    return [[float(x) for x in o] for o in outs]


def main():
    res = {}
    trp, tri, tep, tei, tev = BASE
    lists0 = wb.lists_of(hip.debug_scores(*model("base")), trp, tri, K0)
    # (the replace-the-minimum lists are the scope: a call whose lists are the lane buffers' keeps its sample seeds and gets no bound)
    scope = bool(SPEC["hints"])
    expect = int(wb.hintable(lists0, N, trp, tri, tep).sum()) if scope else 0
    res["expect"] = expect
    res["population"] = {"users": M, "evaluated": int(wb.evaluated_for_ranks(N, K0, trp, tep).sum()), "short": int((lists0 < 0).any(axis=1).sum())}
    drifts = DRIFTS if FULL else ("neg",)
    poisons = wb.POISONS if FULL else ("duplicates", "test_items")
    e = next(int(tep[u + 1] - 1) for u in range(M) if tep[u + 1] - tep[u] >= 2 and tei[tep[u + 1] - 1] + 1 < N)
    changed = [a.copy() for a in BASE]
    changed[3][e] += 1
    K2 = 7 if K0 != 7 else 5
    subset = (0, 2, 5, 7, 8)

    # ---- phase 1: the yardstick, warm bounds off, fresh arrays for every call ----
    os.environ["RM_DEBUG_NO_WARM_BOUNDS"] = "1"
    hip.reload_switches()
    ref = {name: call(Split(BASE), name) for name in ("base",) + tuple(drifts)}
    if FULL:
        ref["changed"] = call(Split(changed), "base")
        ref["K2"] = call(Split(BASE), "base", K=K2)
        ref["subset"] = call(Split(BASE), "base", metrics=subset)
        ref["noise"] = call(Split(BASE), "base", noise=True)
    sp = Split(BASE)
    res["off"] = {"hinted": [call(sp, "base")[2] for _ in range(3)]}
    del os.environ["RM_DEBUG_NO_WARM_BOUNDS"]
    hip.reload_switches()

    # ---- the same model twice, then a third time ----
    sp = first_use()
    got = [call(sp, "base") for _ in range(3)]
    res["same"] = {"reused": [g[1] for g in got], "hinted": [g[2] for g in got], "equal": [equal(g, ref["base"]) for g in got], "outputs": floats(got[2][0])}

    # ---- drift: another model on the lists of the base model, then the base model on the lists of that one ----
    res["drift"] = {}
    for name in drifts:
        sp = first_use()
        a, b, c = call(sp, "base"), call(sp, name), call(sp, "base")
        res["drift"][name] = {"reused": [a[1], b[1], c[1]], "hinted": [a[2], b[2], c[2]], "equal": [equal(a, ref["base"]), equal(b, ref[name]), equal(c, ref["base"])],
                              "outputs": floats(b[0])}

    # ---- standing down: a model whose bounds stay below the positives' makes the next pass skip the kernel, the one after tries again ----
    sp = first_use()
    seq = [call(sp, name) for name in ("base", "neg", "base", "base", "base", "neg", "neg", "neg", "neg", "neg", "base")]
    res["stand_down"] = {"reused": [g[1] for g in seq], "hinted": [g[2] for g in seq],
                         "equal": [equal(g, ref[name]) for g, name in zip(seq, ("base", "neg", "base", "base", "base", "neg", "neg", "neg", "neg", "neg", "base"))]}
    names = ["base", "neg"] * 6                        # ... and a model that never suits the lists it is given: the pauses double
    sp = first_use()
    seq = [call(sp, name) for name in names]
    res["back_off"] = {"hinted": [g[2] for g in seq], "equal": [equal(g, ref[name]) for g, name in zip(seq, names)]}

    # ---- poisoned advice, through the debug entry ----
    res["poison"] = {}
    for kind in poisons:
        ids, users = wb.poisoned(kind, lists0, N, trp, tri, tep, tei)
        sp = first_use()
        a = call(sp, "base")
        if scope:
            hip.set_list_ids(ids)
        b = call(sp, "base")
        res["poison"][kind] = {"users": int(users.shape[0]), "restated": int(wb.hintable(ids, N, trp, tri, tep).sum()) if scope else 0,
                               "hinted": [a[2], b[2]], "equal": [equal(a, ref["base"]), equal(b, ref["base"])], "outputs": floats(b[0])}

    # ---- what voids the lists ----
    if FULL:
        v = res["void"] = {}
        sp = first_use()
        a = call(sp, "base"); sp.poke(3, e, changed[3][e]); b = call(sp, "base"); c = call(sp, "base")
        v["changed_test_item"] = {"reused": [a[1], b[1], c[1]], "hinted": [a[2], b[2], c[2]], "equal": [equal(a, ref["base"]), equal(b, ref["changed"]), equal(c, ref["changed"])]}
        sp = first_use()
        a, b, c, d = call(sp, "base"), call(sp, "base", K=K2), call(sp, "base"), call(sp, "base")
        v["other_K"] = {"reused": [a[1], b[1], c[1], d[1]], "hinted": [a[2], b[2], c[2], d[2]],
                        "equal": [equal(a, ref["base"]), equal(b, ref["K2"]), equal(c, ref["base"]), equal(d, ref["base"])]}
        sp = first_use()
        a, b, c = call(sp, "base"), call(sp, "base", metrics=subset), call(sp, "base")
        v["other_request"] = {"reused": [a[1], b[1], c[1]], "hinted": [a[2], b[2], c[2]], "equal": [equal(a, ref["base"]), equal(b, ref["subset"]), equal(c, ref["base"])]}
        sp = first_use()
        a = call(sp, "base")
        assert hip.load().rm_release_workspace() == 0
        b, c = call(sp, "base"), call(sp, "base")
        v["release"] = {"reused": [a[1], b[1], c[1]], "hinted": [a[2], b[2], c[2]], "equal": [equal(x, ref["base"]) for x in (a, b, c)], "outputs": floats(c[0])}
        sp = first_use()
        a, b, c, d = call(sp, "base"), call(sp, "base", noise=True), call(sp, "base"), call(sp, "base")
        v["tie_noise_between"] = {"reused": [a[1], b[1], c[1], d[1]], "hinted": [a[2], b[2], c[2], d[2]],
                                  "equal": [equal(a, ref["base"]), equal(b, ref["noise"]), equal(c, ref["base"]), equal(d, ref["base"])]}
        # the hook refuses lists it does not know: none kept (the workspace is gone), another shape
        sp = first_use()
        assert hip.load().rm_release_workspace() == 0
        refused = []
        for ids in (lists0, lists0[:, :K0 - 1] if K0 > 1 else lists0[:M - 1]):
            try:
                hip.set_list_ids(ids)
                refused.append(False)
            except ValueError:
                refused.append(True)
            call(sp, "base")
        v["hook_refuses"] = refused
    print(json.dumps(res))


if __name__ == "__main__":
    torch.cuda.set_device(0)
    hip.load()
    hip.set_device(0)
    main()
