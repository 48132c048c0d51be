#!/usr/bin/env python3
"""Generates tests/golden/api/entry_errors.json: what the C-ABI's metric / list entries answer to bad arguments.

For each of the sixteen entries rm_{calc_metrics,calc_metrics_scores,recommend,recommend_scores}[_dev]_{f32,f64} and rm_rank_{f32,f64}
one small valid call is spoiled by every defect that applies to the entry, alone, and by every pair of two defects together.  The
return code and the exact rm_last_error() text of every case answered with RM_ERR_INVALID are stored: which message wins when two
things are wrong is part of the record.  tests/test_entry_errors_cpu.py replays the table.

Run it on a box WITHOUT a device (argument errors are decided before one is asked for; what passes them ends in RM_ERR_HIP there
and is not recorded), against the library whose answers are to be pinned:

    python tests/golden/make_entry_errors.py

The device entries are handed host addresses: no recorded case gets as far as using them.

Cases left out by rule (`left_out`), not by trying them:
* a defect in the contents of an index-pointer array together with that array being null -- there is nothing to spoil;
* two values of K at once.
No remaining case makes the library read through a null pointer: the host entries look at `Xtest_csr_p[m]` and walk the index
pointers only after the null checks of those arrays (and after `m < 0`), and the device entries never read an array on the host.
"""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "api", "entry_errors.json")

RM_ERR_INVALID = 1
M, N, KF, K = 3, 8, 4, 2
SENTINEL = 7

# entry -> (scores instead of factors, lists instead of metrics, rm_rank, host form)
FAMILIES = {
    "rm_calc_metrics": (False, False, False, True), "rm_calc_metrics_dev": (False, False, False, False),
    "rm_rank": (False, False, True, True),
    "rm_calc_metrics_scores": (True, False, False, True), "rm_calc_metrics_scores_dev": (True, False, False, False),
    "rm_recommend": (False, True, False, True), "rm_recommend_dev": (False, True, False, False),
    "rm_recommend_scores": (True, True, False, True), "rm_recommend_scores_dev": (True, True, False, False),
}
SUFFIXES = {"f32": np.float32, "f64": np.float64}


def base_state(entry, dtype):
    """the arguments of a valid call: 3 users, 8 items, 4 factors, K = 2, every output given (NDCG with its test values)"""
    scores, lists, rank, host = FAMILIES[entry]
    st = dict(A=np.arange(M * KF, dtype=dtype).reshape(M, KF), B=np.arange(N * KF, dtype=dtype).reshape(N, KF), lda=KF, ldb=KF,
              S=np.arange(M * N, dtype=dtype).reshape(M, N), lds=N, m=M, n=N, k=KF, K=K,
              train_p=np.array([0, 1, 2, 3], np.int32), train_i=np.array([0, 1, 2], np.int32), nnz_train=3,
              test_p=np.array([0, 1, 2, 3], np.int32), test_i=np.array([5, 6, 7], np.int32), test_v=np.ones(3, dtype), nnz_test=3)
    if lists or rank:
        st.update(idx=np.full((M, K), SENTINEL, np.int32), score=np.full((M, K), SENTINEL, dtype), status=np.full(M, SENTINEL, np.int32))
    if rank:
        st.update(pos_rank=np.full(3, SENTINEL, np.int64))
    elif not lists:
        st.update(outs=[np.full(M, SENTINEL, dtype) for _ in range(10)])
    return st


def _null(name):
    return lambda st: st.__setitem__(name, None)


def _set(name, value):
    return lambda st: st.__setitem__(name, value)


def _first_negative(name):
    def f(st):
        st[name] = st[name].copy()
        st[name][0] = -1
    return f


def _decreasing(name):                        # row 1 ends in front of its start
    def f(st):
        st[name] = st[name].copy()
        st[name][2] = 0
    return f


def defects_of(entry):
    """name -> function that spoils the state, in a fixed order"""
    scores, lists, rank, host = FAMILIES[entry]
    metrics = not lists
    d = {}
    for name in (["S"] if scores else ["A", "B"]) + ["train_p", "train_i"] + (["test_p", "test_i"] if metrics else []):
        d[name + "=null"] = _null(name)
    if metrics and not rank:
        d["test_v=null with NDCG requested"] = _null("test_v")
    for name in (["idx", "status"] if lists else ["idx", "score", "pos_rank", "status"] if rank else []):
        d[name + "=null"] = _null(name)
    d["m<0"] = _set("m", -1)
    d["n=0"] = _set("n", 0)
    if not scores:
        d["k=0"] = _set("k", 0)
    for name, v in (("K=0", 0), ("K=-1", -1), ("K=n+1", N + 1)):
        d[name] = _set("K", v)
    for name, v in ([("lds", N - 1)] if scores else [("lda", KF - 1), ("ldb", KF - 1)]):
        d[name + " one too small"] = _set(name, v)
    for name in ["train"] + (["test"] if metrics else []):
        if host:
            d[name + "_p[0]<0"] = _first_negative(name + "_p")
            d[name + "_p decreasing at row 1"] = _decreasing(name + "_p")
        else:
            d["nnz_" + name + "<0"] = _set("nnz_" + name, -1)
    return d


def left_out(defects):
    """the rule of the module's docstring"""
    if sum(d.startswith("K=") for d in defects) > 1:
        return True
    for arr in ("train_p", "test_p"):
        if arr + "=null" in defects and any(d.startswith(arr + "[") or d.startswith(arr + " ") for d in defects):
            return True
    return False


def cases_of(entry):
    names = list(defects_of(entry))
    combos = [(a,) for a in names] + list(itertools.combinations(names, 2))
    return [c for c in combos if not left_out(c)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# parameter of include/recometrics_hip.h -> key of the state, where they differ (the lists' exclusion matrix is the state's train matrix)
STATE_KEY = {"Xtrain_csr_p": "train_p", "Xtrain_csr_i": "train_i", "Xexcl_csr_p": "train_p", "Xexcl_csr_i": "train_i", "nnz_excl": "nnz_train",
             "Xtest_csr_p": "test_p", "Xtest_csr_i": "test_i", "Xtest_csr": "test_v", "k_metrics": "K", "k_top": "K", "topk_idx": "idx", "topk_score": "score"}


def call(lib, entry, suffix, defects):
    """the spoiled call, its arguments ordered by the binding's table of signatures; returns (rc, message, the output arrays it was given)"""
    from recometrics_amd import _binding
    st = base_state(entry, SUFFIXES[suffix])
    table = defects_of(entry)
    for d in defects:
        table[d](st)
    outs = [st[name] for name in ("idx", "score", "pos_rank", "status") if name in st] + st.get("outs", [])
    st.update(zip(_binding.OUTPUTS, st.pop("outs", [])))
    st.update(cumulative=0, break_ties_with_noise=1, consider_cold_start=1, min_items_pool=2, min_pos_test=1, nthreads=1,
              seed=1 if entry == "rm_rank" else 5, stream=None)
    values = [st[STATE_KEY.get(name, name)] for name, _ in _binding.SIGNATURES[entry + "_" + suffix][0]]
    rc = getattr(lib, entry + "_" + suffix)(*[_p(v) if v is None or isinstance(v, np.ndarray) else v for v in values])
    return rc, (lib.rm_last_error() or b"").decode(), [o for o in outs if o is not None]


def dump(data, path):
    """one line per message and per case"""
    js = lambda x: json.dumps(x, sort_keys=True)
    with open(path, "w") as f:
        f.write('{"format": %s,\n "messages": [\n  %s],\n "cases": {\n' % (js(data["format"]), ",\n  ".join(js(m) for m in data["messages"])))
        entries = sorted(data["cases"])
        for e in entries:
            rows = data["cases"][e]
            f.write('  %s: {\n   %s}%s\n' % (js(e), ",\n   ".join("%s: %s" % (js(c), js(rows[c])) for c in sorted(rows)), "" if e == entries[-1] else ","))
        f.write(" }\n}\n")


def main():
    from recometrics_amd import _binding
    lib = _binding.load()
    assert _binding.device_count() <= 0, "run this without a device: the device entries are handed host addresses"
    messages, table, count = [], {}, 0
    for entry in FAMILIES:
        for suffix in SUFFIXES:
            rows = table.setdefault(entry + "_" + suffix, {})
            for defects in cases_of(entry):
                rc, msg, _ = call(lib, entry, suffix, defects)
                if rc != RM_ERR_INVALID:
                    continue
                if msg not in messages:
                    messages.append(msg)
                rows[" + ".join(defects)] = [rc, messages.index(msg)]
                count += 1
    assert count >= 400, count
    dump({"format": "cases[entry][defects joined by ' + '] = [return code, index into messages]", "messages": messages, "cases": table}, OUT)
    print("%d cases, %d messages -> %s" % (count, len(messages), OUT))


if __name__ == "__main__":
    main()
