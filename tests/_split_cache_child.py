"""Child process of tests/test_hip_split_cache.py: torch owns the device memory (loaded before the library), the calls go through
_binding.calc_metrics_device.  Usage: python _split_cache_child.py f32|f64 -- prints one JSON line, scenario -> findings.

Phase 1 runs every call the scenarios make with RM_DEBUG_NO_SPLIT_CACHE=1, each on freshly allocated arrays: the yardstick.
Phase 2 switches the reuse on (one reload of the switches, which voids whatever a context kept) and plays the scenarios; every
output array of every call must equal its yardstick bit for bit."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from recometrics_amd import _binding as hip          # noqa: E402
from recometrics_amd.synth import make_factors, make_interactions          # noqa: E402
from _util import same_bits          # noqa: E402

M, N, KF, MEAN = 300, 700, 16, 120
ALL = tuple(range(10))
DT = {"f32": np.float32, "f64": np.float64}[sys.argv[1] if __name__ == "__main__" else "f32"]
OTHER = np.float64 if DT == np.float32 else np.float32

dev = torch.device("cuda", 0)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def split_arrays(dtype=DT):
    """make_interactions, mean 120, with HALF of a row held out: at the default 30 % the longest test row of this shape has 52 entries
    (rows are capped at n / 4 = 175 items) and nobody is streamed; at 50 % some rows have more than 63.  Four users are hollowed out
    afterwards -- the draws give everybody both rows --: two lose their train row, two their test row, one of them both."""
    trp, tri, tep, tei, tev = make_interactions(M, N, MEAN, dtype, seed=5, test_fraction=0.5)

    def without_rows(p, arrays, users):
        keep = np.ones(p[-1], bool)
        for u in users:
            keep[p[u]:p[u + 1]] = False
        counts = np.diff(p)
        counts[list(users)] = 0
        q = np.zeros_like(p)
        np.cumsum(counts, out=q[1:])
        return [q] + [a[keep] for a in arrays]
    trp, tri = without_rows(trp, [tri], (17, 40))
    tep, tei, tev = without_rows(tep, [tei, tev], (40, 77))
    return [trp, tri, tep, tei, tev]


def factors(i, dtype=DT):
    return make_factors(M, N, KF, dtype, seed=100 + i)


class Split:
    """the five arrays of a split in device memory (and what they hold, on the host)"""
    def __init__(self, arrays, offset=False):
        self.np = [a.copy() for a in arrays]
        self.d = [t(a) for a in self.np]
        self.other_tev = None               # the test values in the other precision (OPTIONS' dtype step): one array for both of its calls
        if offset:
            # the four index arrays 4 bytes behind an allocation: not 16-byte aligned (k_split_same compares such an array word by word)
            for i in range(4):
                room = torch.empty(self.np[i].shape[0] + 1, dtype=torch.int32, device=dev)
                room[1:] = self.d[i]
                self.d[i] = room[1:]
                assert self.d[i].data_ptr() % 16 == 4

    def poke(self, which, at, value):
        """changes one element in place: same pointers, same sizes"""
        self.np[which][at] = value
        self.d[which][at] = value.item() if hasattr(value, "item") else value
        torch.cuda.synchronize()


def call(sp, ab, K=10, metrics=ALL, cumulative=False, noise=False, dtype=DT):
    """one metric call; returns (outputs, split_reused) or ("error", message)"""
    A, B = (t(x) for x in factors(ab, dtype))
    tt = torch.float32 if dtype == np.float32 else torch.float64
    outs = [torch.full((M * (K if cumulative and i < 8 else 1),), -7.0, dtype=tt, device=dev) if i in metrics else None for i in range(10)]
    if sp.d[4].dtype != tt and sp.other_tev is None:
        sp.other_tev = sp.d[4].to(tt)
    tev = sp.d[4] if sp.d[4].dtype == tt else sp.other_tev
    try:
        hip.calc_metrics_device(dtype, A.data_ptr(), KF, B.data_ptr(), KF, M, N, KF, sp.d[0].data_ptr(), sp.d[1].data_ptr(), sp.np[1].shape[0],
                                sp.d[2].data_ptr(), sp.d[3].data_ptr(), tev.data_ptr(), sp.np[3].shape[0], K,
                                [o.data_ptr() if o is not None else 0 for o in outs], cumulative=cumulative, break_ties_with_noise=noise, seed=3)
    except ValueError as e:
        return "error", str(e)
    torch.cuda.synchronize()
    return [o.cpu().numpy() if o is not None else None for o in outs], hip.timings().get("split_reused")


def equal(got, want):
    if got[0] == "error" or want[0] == "error":
        return got[0] == want[0] and got[1] == want[1]
    return all((g is None and w is None) or bool(same_bits(g, w).all()) for g, w in zip(got[0], want[0]))


BASE = split_arrays()


# ---- the in-place changes of scenario 2 and the defects of scenario 3: (which array, index, new value) from the base arrays ----
def _row_end_bump(p, idx):
    """last entry of a row with at least two entries whose id can grow by one: the row stays sorted"""
    for u in range(M):
        if p[u + 1] - p[u] >= 2 and idx[p[u + 1] - 1] + 1 < N:
            return int(p[u + 1] - 1), np.int32(idx[p[u + 1] - 1] + 1)
    raise AssertionError("no such row")


def _owner_move(p, idx):
    """row u hands its last entry to row u + 1: p[u + 1] moves down by one.  Where some row u + 1 stays sorted by it (it is empty, or
    the entry is below its first) that pair is taken; else the first pair with entries, and the row that grew is unsorted -- the call
    then sorts a copy, with the reuse on as with it off"""
    fits = [u for u in range(M - 1) if p[u + 1] - p[u] >= 2 and (p[u + 2] == p[u + 1] or idx[p[u + 1] - 1] < idx[p[u + 1]])]
    u = fits[0] if fits else next(u for u in range(M - 1) if p[u + 1] - p[u] >= 2 and p[u + 2] > p[u + 1])
    return u + 1, np.int32(p[u + 1] - 1)


def changes():
    trp, tri, tep, tei, tev = BASE
    e, v = _row_end_bump(tep, tei)
    out = {"a_test_item": [(3, e, v)], "b_test_value": [(4, 7, DT(tev[7] + 1))]}
    e, v = _row_end_bump(trp, tri)
    out["c_train_index"] = [(1, e, v)]
    out["d_test_p"] = [(2,) + _owner_move(tep, tei)]
    out["e_train_p"] = [(0,) + _owner_move(trp, tri)]
    # the very last element of an index array whose length is no multiple of four: behind the last whole 16-byte piece
    which = next(w for w in (1, 3) if BASE[w].shape[0] % 4)
    last = int(BASE[which][-1])
    out["f_last_word"] = [(which, BASE[which].shape[0] - 1, np.int32(last + 1 if last + 1 < N else last - 1))]
    return out


def defects():
    trp, tri, tep, tei, tev = BASE
    u = next(u for u in range(M) if tep[u + 1] - tep[u] >= 2)
    a = int(tep[u])
    return {"index_n": [(3, int(tep[123]), np.int32(N))],
            "descending": [(3, a, np.int32(tei[a + 1])), (3, a + 1, np.int32(tei[a]))]}


OPTIONS = [dict(K=7), dict(metrics=(0, 2, 5, 7)), dict(metrics=(0, 1, 2, 3, 4, 5, 6, 7, 9)), dict(cumulative=True), dict(noise=True), dict(),
           dict(dtype=OTHER), dict()]


def recommend(sp, ab):
    A, B = (t(x) for x in factors(ab))
    tt = torch.float32 if DT == np.float32 else torch.float64
    idx = torch.full((M * 10,), -1, dtype=torch.int32, device=dev); sc = torch.zeros(M * 10, dtype=tt, device=dev)
    st = torch.zeros(M, dtype=torch.int32, device=dev)
    hip.recommend_device(DT, A.data_ptr(), KF, B.data_ptr(), KF, M, N, KF, sp.d[0].data_ptr(), sp.d[1].data_ptr(), sp.np[1].shape[0], 10,
                         idx.data_ptr(), sc.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    return [idx.cpu().numpy().astype(DT), sc.cpu().numpy(), st.cpu().numpy().astype(DT)], None


def from_scores(sp, ab):
    A, B = factors(ab)
    S = t((A.astype(np.float64) @ B.astype(np.float64).T).astype(DT))
    tt = torch.float32 if DT == np.float32 else torch.float64
    outs = [torch.full((M,), -7.0, dtype=tt, device=dev) for _ in range(10)]
    hip.calc_metrics_scores_device(DT, S.data_ptr(), N, M, N, sp.d[0].data_ptr(), sp.d[1].data_ptr(), sp.np[1].shape[0], sp.d[2].data_ptr(),
                                   sp.d[3].data_ptr(), sp.d[4].data_ptr(), sp.np[3].shape[0], 10, [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], None


def first_use():
    """a split nothing is kept of: torch hands the addresses of the arrays a scenario has dropped to the next one's, and a context
    that still keeps the split of those addresses would reuse it on the first call (rightly so, when the contents are equal); a
    reload of the switches voids what the contexts keep"""
    hip.reload_switches()
    return Split(BASE)


def changed(ch):
    arrays = [a.copy() for a in BASE]
    for which, at, value in ch:
        arrays[which][at] = value
    return arrays


def main():
    res = {}
    # ---- phase 1: the yardstick, reuse off, fresh arrays for every call ----
    os.environ["RM_DEBUG_NO_SPLIT_CACHE"] = "1"
    hip.reload_switches()
    ref = {("base", i): call(Split(BASE), i) for i in range(3)}
    assert all(r[1] in (-1, None) or r[0] == "error" for r in ref.values()), "the reuse is off: split_reused must say so"
    for name, ch in list(changes().items()) + list(defects().items()):
        ref[(name, 2)] = call(Split(changed(ch)), 2)
    for j, kw in enumerate(OPTIONS):
        ref[("opt", j)] = call(Split(BASE), j % 3, **kw)
    ref["reco"] = recommend(Split(BASE), 1)
    ref["scores"] = from_scores(Split(BASE), 1)
    res["yardstick_errors"] = {str(k): v[1] for k, v in ref.items() if v[0] == "error"}
    del os.environ["RM_DEBUG_NO_SPLIT_CACHE"]
    hip.reload_switches()

    # ---- 1: three calls on one split, three models ----
    sp = first_use()
    got = [call(sp, i) for i in range(3)]
    res["three_calls"] = {"reused": [g[1] for g in got], "equal": [equal(g, ref[("base", i)]) for i, g in enumerate(got)]}
    # (the third call's outputs, a call that ran on the kept split, for the comparison with the oracle; floats survive JSON exactly)
    res["reused_outputs"] = [[float(x) for x in o] for o in got[2][0]]

    # ---- 2: contents changed in place; 3: contents made invalid in place ----
    for group, table in (("changed", changes()), ("invalid", defects())):
        res[group] = {}
        for name, ch in table.items():
            sp = first_use()
            warm = [call(sp, 0), call(sp, 1)]
            for which, at, value in ch:
                sp.poke(which, at, value)
            g = call(sp, 2)
            res[group][name] = {"warm_reused": [w[1] for w in warm], "warm_equal": [equal(w, ref[("base", i)]) for i, w in enumerate(warm)],
                                "reused": g[1], "equal": equal(g, ref[(name, 2)]), "error": g[1] if g[0] == "error" else None}
    # ... and the same with the caller's index arrays not 16-byte aligned
    res["unaligned"] = {}
    for name in ("a_test_item", "c_train_index", "f_last_word"):
        hip.reload_switches()
        sp = Split(BASE, offset=True)
        warm = [call(sp, 0), call(sp, 1)]
        for which, at, value in changes()[name]:
            sp.poke(which, at, value)
        g = call(sp, 2)
        res["unaligned"][name] = {"warm_reused": [w[1] for w in warm], "warm_equal": [equal(w, ref[("base", i)]) for i, w in enumerate(warm)],
                                  "reused": g[1], "equal": equal(g, ref[(name, 2)])}
    # (the library is fine afterwards)
    res["after_invalid"] = equal(call(first_use(), 0), ref[("base", 0)])

    # ---- 4: same arrays, the request changes from call to call (each request twice: the second may reuse what the first kept) ----
    sp = first_use()
    res["options"] = []
    for j, kw in enumerate(OPTIONS):
        a, b = call(sp, j % 3, **kw), call(sp, j % 3, **kw)
        res["options"].append({"kw": {k: (str(v) if k == "dtype" else v) for k, v in kw.items()}, "equal": [equal(a, ref[("opt", j)]), equal(b, ref[("opt", j)])],
                               "reused": [a[1], b[1]]})

    # ---- 5: the workspace released between two calls ----
    sp = first_use()
    a = call(sp, 0)
    assert hip.load().rm_release_workspace() == 0
    b = call(sp, 1)
    c = call(sp, 2)
    res["release"] = {"reused": [a[1], b[1], c[1]], "equal": [equal(a, ref[("base", 0)]), equal(b, ref[("base", 1)]), equal(c, ref[("base", 2)])]}

    # ---- 6: lists and a score matrix between two metric calls on the same split ----
    sp = first_use()
    a = call(sp, 0); r = recommend(sp, 1); b = call(sp, 1); s = from_scores(sp, 1); c = call(sp, 2); d = call(sp, 0)
    res["between"] = {"reused": [a[1], b[1], c[1], d[1]],
                      "equal": [equal(a, ref[("base", 0)]), equal(r, ref["reco"]), equal(b, ref[("base", 1)]), equal(s, ref["scores"]),
                                equal(c, ref[("base", 2)]), equal(d, ref[("base", 0)])]}
    print(json.dumps(res))


if __name__ == "__main__":
    torch.cuda.set_device(0)
    hip.load()
    hip.set_device(0)
    main()
