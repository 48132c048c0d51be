#!/usr/bin/env python3
"""Generates tests/golden/api/python_errors.json: what the four public functions of recometrics_amd/__init__.py do with their
arguments BEFORE the library is touched -- which exception (type and exact text) a bad call gets, which warnings fire, and what a
good call hands to the binding and makes of its answer.

For each of calc_reco_metrics, calc_reco_metrics_from_scores, recommend_topk and recommend_topk_from_scores one small valid call (6
users, 9 items, 3 factors, k = 3, nthreads = 2) is changed by every entry of `changes_of()`, alone, and by every pair of two.  An
entry is either a defect -- one per `_fail_if`, `assert` and `warn` of the function and of the helpers it calls -- or an input variant
that changes what reaches the binding (another dtype or memory order, int64 index arrays, another SciPy format, `X_train=None`,
`item_biases`, `users`, `as_df`, `cumulative`, `all_metrics`, ...).  Which message wins when two things are wrong is part of the record.

The library is not loaded: `_binding.has_openmp` is a stub and the four host wrappers are replaced by a recorder.  Per case:
  raises     [exception type, exact text]                                   (the distinction AssertionError / ValueError is kept)
  warnings   the sorted warning texts
  binding    what reached the wrapper, by the parameter names of the wrapper's signature: arrays as
             [dtype, shape, strides in elements, crc32 of the contents], scalars as [type, value], `want` as it is, `outs` as a list
             of arrays without their contents (storage still to be written)
  result     what the function returned: a frame's columns, shape, dtypes, contents and whether its storage IS the `outs` of the
             call; a dict's entries; a tuple's
The call without a change is stored in full; every other passing case stores only what differs from it.  The file states every
description, text and result once (`values`); records and cases refer to them by place (`encode` / `decode`).

    python tests/golden/make_python_errors.py

Cases left out by rule (`left_out`), not by trying them:
* two changes that set the same argument (two values of one argument at once);
* in calc_reco_metrics, an `X_test` of 2^31 - 1 rows together with the item-bias-only mode: the function would allocate a column of
  ones for every one of those rows before it looks at their number.
A negative `nthreads` that stays in range is not a case: it resolves through multiprocessing.cpu_count(), a property of the machine.
"""
import functools
import inspect
import itertools
import json
import os
import sys
import warnings
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "api", "python_errors.json")

M, N, KF, K = 6, 9, 3, 3
HUGE = 2 ** 31 - 1
# public function -> the host wrapper of _binding it ends in
FUNCTIONS = {"calc_reco_metrics": "calc_metrics", "calc_reco_metrics_from_scores": "calc_metrics_scores",
             "recommend_topk": "recommend", "recommend_topk_from_scores": "recommend_scores"}
OPENMP = "_openmp"                      # key of the state that is not an argument: what the has_openmp stub answers


def _dense(rows, cols, dtype=np.float32, step=7):
    return (((np.arange(rows * cols) * step) % 11 - 5) / 4).astype(dtype).reshape(rows, cols)


def _csr(rows=M, cols=N, shift=0, index=np.int32, values=np.float64):
    """two entries per row, at columns that wrap around: some rows are not sorted"""
    from scipy.sparse import csr_array
    u = np.repeat(np.arange(rows), 2)
    col = (3 * u + shift + 4 * (np.arange(2 * rows) % 2)) % cols
    return csr_array(((1 + np.arange(2 * rows) % 3).astype(values), col.astype(index), np.arange(0, 2 * rows + 1, 2).astype(index)),
                     shape=(rows, cols))


def _coo_of_shape(rows, cols):
    from scipy.sparse import coo_array
    return coo_array((np.ones(2), (np.array([0, 1]), np.array([1, 2]))), shape=(rows, cols))


def _empty_csr():
    from scipy.sparse import csr_array
    return csr_array((M, N), dtype=np.float64)


def _strided(X):
    wide = np.zeros((X.shape[0], X.shape[1] + 5), X.dtype)
    wide[:, 2:2 + X.shape[1]] = X
    return wide[:, 2:2 + X.shape[1]]


def _series(x):
    import pandas as pd
    return pd.Series(x)


BIASES = _dense(1, N, np.float32, step=3).reshape(-1)


def base_kwargs(function):
    """the arguments of the valid call"""
    if function == "calc_reco_metrics":
        return dict(X_train=_csr(), X_test=_csr(shift=1), A=_dense(M, KF), B=_dense(N, KF, step=5), k=K, nthreads=2, **{OPENMP: True})
    if function == "calc_reco_metrics_from_scores":
        return dict(X_train=_csr(), X_test=_csr(shift=1), scores=_dense(M, N), k=K, nthreads=2)
    if function == "recommend_topk":
        return dict(A=_dense(M, KF), B=_dense(N, KF, step=5), k=K)
    return dict(scores=_dense(M, N), k=K)


def _dense_changes(name, few):
    """variants of a dense argument (`few`: the layouts only) -- what reaches the binding changes, the call stays valid"""
    d = {name + " float64": lambda kw: kw[name].astype(np.float64), name + " Fortran order": lambda kw: np.asfortranarray(kw[name]),
         name + " strided rows": lambda kw: _strided(kw[name])}
    if not few:
        d.update({name + " float16": lambda kw: kw[name].astype(np.float16), name + " int32": lambda kw: (4 * kw[name]).astype(np.int32),
                  name + " reversed rows": lambda kw: kw[name][::-1]})
    return {label: ((name,), (lambda f: lambda kw: kw.__setitem__(name, f(kw)))(f)) for label, f in d.items()}


def _set(**values):
    return tuple(values), lambda kw: kw.update(values)


def _factor_changes():
    d = {"A=None alone": _set(A=None), "B=None alone": _set(B=None), "A=B=None": _set(A=None, B=None),
         "A a list": (("A",), lambda kw: kw.update(A=kw["A"].tolist())), "B a list": (("B",), lambda kw: kw.update(B=kw["B"].tolist())),
         "A 1-d": _set(A=_dense(1, M).reshape(-1)), "B 3-d": _set(B=_dense(N, KF).reshape(N, KF, 1)),
         "A one more column": _set(A=_dense(M, KF + 1)), "A no columns": _set(A=_dense(M, 0)), "B no columns": _set(B=_dense(N, 0)),
         "A no rows": _set(A=_dense(0, KF)), "B no rows": _set(B=_dense(0, KF))}
    d.update(_dense_changes("A", False))
    d.update(_dense_changes("B", True))
    return d


def _bias_changes():
    return {"item_biases": _set(item_biases=BIASES), "item_biases a Series": (("item_biases",), lambda kw: kw.update(item_biases=_series(BIASES))),
            "item_biases a column": _set(item_biases=BIASES.reshape(-1, 1)), "item_biases float64": _set(item_biases=BIASES.astype(np.float64)),
            "item_biases a list": _set(item_biases=BIASES.tolist()), "item_biases 3-d": _set(item_biases=BIASES.reshape(3, 3, 1)),
            "item_biases empty": _set(item_biases=BIASES[:0]), "item_biases too few": _set(item_biases=BIASES[:N - 1]),
            "item_biases too many": _set(item_biases=np.append(BIASES, BIASES[:2])),
            "item_biases alone": _set(A=None, B=None, item_biases=BIASES)}


def _score_changes():
    d = {"scores a list": (("scores",), lambda kw: kw.update(scores=kw["scores"].tolist())), "scores 1-d": _set(scores=_dense(1, M * N).reshape(-1)),
         "scores 3-d": _set(scores=_dense(M, N).reshape(M, N, 1)), "scores complex": _set(scores=_dense(M, N).astype(np.complex64)),
         "scores of objects": _set(scores=_dense(M, N).astype(object)), "scores one more row": _set(scores=_dense(M + 1, N)),
         "scores one column fewer": _set(scores=_dense(M, N - 1)), "scores no rows": _set(scores=_dense(0, N)), "scores no columns": _set(scores=_dense(M, 0)),
         "scores bool": (("scores",), lambda kw: kw.update(scores=kw["scores"] > 0))}
    d.update(_dense_changes("scores", False))
    return d


def _split_changes():
    """X_train / X_test of the metric calls"""
    return {"X_train=None": _set(X_train=None), "X_train dense": _set(X_train=_csr().toarray()), "X_train one more column": _set(X_train=_csr(cols=N + 1)),
            "X_train one row fewer": _set(X_train=_csr(rows=M - 1)), "X_train two more rows": _set(X_train=_csr(rows=M + 2)),
            "X_train int64 indices": _set(X_train=_csr(index=np.int64)), "X_train COO": _set(X_train=_csr().tocoo()),
            "X_train CSC float32": _set(X_train=_csr(values=np.float32).tocsc()),
            "X_test dense": _set(X_test=_csr(shift=1).toarray()), "X_test 2^31-1 rows": _set(X_test=_coo_of_shape(HUGE, N)),
            "X_test 2^31-1 columns": _set(X_test=_coo_of_shape(M, HUGE)), "X_test nothing stored": _set(X_test=_empty_csr()),
            "X_test no rows": _set(X_test=_csr(rows=0, shift=1)), "X_test no columns": _set(X_test=_csr(shift=1)[:, :0]),
            "X_test int64 indices": _set(X_test=_csr(shift=1, index=np.int64)), "X_test COO": _set(X_test=_csr(shift=1).tocoo()),
            "X_test float32 values": _set(X_test=_csr(shift=1, values=np.float32)), "X_test int64 values": _set(X_test=_csr(shift=1, values=np.int64)),
            "X_test one more row": _set(X_test=_csr(rows=M + 1, shift=1)), "X_test one column fewer": _set(X_test=_csr(cols=N - 1, shift=1))}


def _request_changes(function):
    d = {"no metric": _set(precision=False, average_precision=False, ndcg=False), "recall alone": _set(precision=False, average_precision=False, ndcg=False, recall=True),
         "roc_auc alone": _set(precision=False, average_precision=False, ndcg=False, roc_auc=True), "hit, rr, pr_auc too": _set(hit=True, rr=True, pr_auc=True),
         "all_metrics": _set(all_metrics=True), "as_df=False": _set(as_df=False), "cumulative": _set(cumulative=True), "rename_k=False": _set(rename_k=False),
         "consider_cold_start=False": _set(consider_cold_start=False), "k=0": _set(k=0), "k=1": _set(k=1), "k=n+1": _set(k=N + 1), "k=2.9": _set(k=2.9),
         "min_pos_test=0": _set(min_pos_test=0), "min_pos_test=2": _set(min_pos_test=2), "min_items_pool=0": _set(min_items_pool=0),
         "min_items_pool=3": _set(min_items_pool=3), "nthreads=0": _set(nthreads=0), "nthreads=1": _set(nthreads=1), "nthreads=-100000": _set(nthreads=-100000)}
    if function == "calc_reco_metrics":
        d.update({"seed=0": _set(seed=0), "seed=7": _set(seed=7), "seed a RandomState": (("seed",), lambda kw: kw.update(seed=np.random.RandomState(3))),
                  "seed a Generator": (("seed",), lambda kw: kw.update(seed=np.random.default_rng(3))),
                  "break_ties_with_noise=False": _set(break_ties_with_noise=False), "built without OpenMP": _set(**{OPENMP: False})})
    return d


def _list_changes(source):
    """k, X_train, users and return_scores of the list calls; `source`: the argument whose rows `users` selects"""
    return {"k=0": _set(k=0), "k=1": _set(k=1), "k=n+1": _set(k=N + 1), "k=2.9": _set(k=2.9), "return_scores=False": _set(return_scores=False),
            "X_train": _set(X_train=_csr()), "X_train dense": _set(X_train=_csr().toarray()), "X_train one more column": _set(X_train=_csr(cols=N + 1)),
            "X_train one more row": _set(X_train=_csr(rows=M + 1)), "X_train int64 indices": _set(X_train=_csr(index=np.int64)),
            "X_train COO": _set(X_train=_csr().tocoo()),
            "users": _set(users=np.array([3, 0, 3, 5])), "users a list": _set(users=[4, 1]), "users int32": _set(users=np.array([2, 2], np.int32)),
            "users empty": _set(users=np.zeros(0, np.int64)), "users an empty list": _set(users=[]),
            "users 2-d": _set(users=np.array([[1, 2]])), "users float": _set(users=np.array([1.0, 2.0])), "users negative": _set(users=np.array([0, -1])),
            "users beyond the rows": _set(users=np.array([0, M])),
            source + " 2^31-1 rows": ((source,), lambda kw: kw.update({source: np.broadcast_to(kw[source][:1], (HUGE, kw[source].shape[1]))}))}


@functools.lru_cache(maxsize=None)
def changes_of(function):
    """label -> (the arguments it sets, function that changes the keyword arguments), in a fixed order"""
    if function == "calc_reco_metrics":
        d = {**_factor_changes(), **_bias_changes(), **_split_changes(), **_request_changes(function),
             "A one row fewer": _set(A=_dense(M - 1, KF)), "A two more rows": _set(A=_dense(M + 2, KF)),
             "B one row fewer": _set(B=_dense(N - 1, KF, step=5)), "B two more rows": _set(B=_dense(N + 2, KF, step=5))}
    elif function == "calc_reco_metrics_from_scores":
        d = {**_score_changes(), **_split_changes(), **_request_changes(function)}
    elif function == "recommend_topk":
        d = {**_factor_changes(), **_bias_changes(), **_list_changes("A"),
             "B 2^31-1 rows": (("B",), lambda kw: kw.update(B=np.broadcast_to(kw["B"][:1], (HUGE, KF))))}
    else:
        d = {**_score_changes(), **_list_changes("scores"),
             "scores 2^31-1 columns": (("scores",), lambda kw: kw.update(scores=np.broadcast_to(kw["scores"][:, :1], (M, HUGE))))}
    return d


def left_out(function, labels):
    """the rules of the module's docstring"""
    table = changes_of(function)
    sets = [set(table[label][0]) for label in labels]
    if len(sets) == 2 and sets[0] & sets[1]:
        return True
    return function == "calc_reco_metrics" and set(labels) == {"X_test 2^31-1 rows", "item_biases alone"}


def cases_of(function):
    names = list(changes_of(function))
    combos = [()] + [(a,) for a in names] + list(itertools.combinations(names, 2))
    return [c for c in combos if not left_out(function, c)]


def _describe(v, contents=True):
    """`contents=False`: of storage that is still to be written"""
    if isinstance(v, np.ndarray):
        return [str(v.dtype), list(v.shape), [s // v.itemsize for s in v.strides]] + ([zlib.crc32(np.ascontiguousarray(v).tobytes())] if contents else [])
    if isinstance(v, (list, tuple)):
        return [_describe(x, contents) for x in v]
    if isinstance(v, dict):
        return {key: _describe(x, contents) for key, x in v.items()}
    if v is None:
        return None
    return [type(v).__name__, v if isinstance(v, (bool, int, float, str)) else repr(v)]


def _recorder(wrapper, seen):
    """stands in for a host wrapper of _binding: notes the arguments under the names of the wrapper's signature; the metric wrappers
    answer as the real ones do (the caller's `outs`, or new arrays: size 0 = not requested, [m, k] when cumulative), every metric
    filled with a value of its own"""
    sig = inspect.signature(wrapper)

    def fake(*args, **kwargs):
        from recometrics_amd import _binding
        got = sig.bind(*args, **kwargs)
        got.apply_defaults()
        seen.update(got.arguments)
        seen["_described"] = {name: v if name == "want" else _describe(v, name != "outs") for name, v in got.arguments.items()}
        if "want" not in got.arguments:
            return "ids", "scores", "status"
        a = got.arguments
        src = a["A"] if "A" in a else a["S"]
        outs = a["outs"]
        if outs is None:
            shape = (src.shape[0], a["k_metrics"]) if a["cumulative"] else (src.shape[0],)
            outs = [np.empty((shape if i < 8 else shape[:1]) if a["want"][name] else ((0, 0) if a["cumulative"] and i < 8 else 0), src.dtype)
                    for i, name in enumerate(_binding.METRIC_ORDER)]
        for i, o in enumerate(outs):
            o[...] = (i + 1) / 16
        return tuple(outs)
    return fake


def _describe_result(res, outs):
    if type(res).__name__ == "DataFrame":
        mine = outs is not None and all(np.shares_memory(res.values, o) for o in outs if o.size)
        return {"frame": {"columns": [str(c) for c in res.columns], "shape": list(res.shape), "dtypes": sorted({str(t) for t in res.dtypes}),
                          "crc": zlib.crc32(np.ascontiguousarray(res.to_numpy()).tobytes()), "is_outs": bool(mine)}}
    if isinstance(res, dict):
        return {"dict": _describe(res)}
    return {"tuple": _describe(res)}


def run(function, labels):
    """the full record of one case"""
    import recometrics_amd
    from recometrics_amd import _binding
    kw = base_kwargs(function)
    table = changes_of(function)
    for label in labels:
        table[label][1](kw)
    openmp = kw.pop(OPENMP, True)
    saved = {name: getattr(_binding, name) for name in list(FUNCTIONS.values()) + ["has_openmp"]}
    seen, rec = {}, {}
    try:
        _binding.has_openmp = lambda: openmp
        for name in FUNCTIONS.values():
            setattr(_binding, name, _recorder(saved[name], seen) if name == FUNCTIONS[function] else None)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                res = getattr(recometrics_amd, function)(**kw)
                if seen:
                    rec["binding"] = seen["_described"]
                rec["result"] = _describe_result(res, seen.get("outs"))
            except Exception as e:                                  # noqa: BLE001 -- whatever the caller would get is the record
                rec["raises"] = [type(e).__name__, str(e)]
        if caught:
            rec["warnings"] = sorted(str(w.message) for w in caught)
    finally:
        for name, f in saved.items():
            setattr(_binding, name, f)
    return rec


def compact(rec, base):
    """a passing case as its difference from the call without a change (`base`: that call's full record)"""
    if "binding" not in rec or rec is base:
        return rec
    out = {key: v for key, v in rec.items() if key not in ("binding", "result")}
    out["binding"] = {name: v for name, v in rec["binding"].items() if base["binding"].get(name, "absent") != v}
    if rec["result"] != base["result"]:
        out["result"] = rec["result"]
    return out


def records_of(function):
    """label -> compact record, for every case of `cases_of`"""
    base = run(function, ())
    assert "binding" in base, base
    return {" + ".join(c): compact(run(function, c) if c else base, base) for c in cases_of(function)}


class _Table(list):
    """distinct JSON values in the order they were first seen; `ref` gives a value's place"""
    def ref(self, x):
        key = json.dumps(x, sort_keys=True)
        places = self.__dict__.setdefault("places", {})
        if key not in places:
            places[key] = len(self)
            self.append(x)
        return places[key]


def encode(records):
    """{function: {label: compact record}} -> the file's content: every [argument, description], text and result is stated once in `values`, a
    record names them by place, and a function's cases name their records by place, in the order of `cases_of`"""
    values, short, cases = _Table(), _Table(), {}
    for function, rows in records.items():
        assert list(rows) == [" + ".join(c) for c in cases_of(function)]
        cases[function] = [short.ref({key: [values.ref(w) for w in v] if key == "warnings" else
                                      [values.ref([name, d]) for name, d in v.items()] if key == "binding" else values.ref(v)
                                      for key, v in rec.items()}) for rec in rows.values()]
    return {"format": "cases[function][i] = place in records of the i-th case of cases_of(function); a record's numbers = places in values",
            "values": list(values), "records": list(short), "cases": cases}


def decode(data, function):
    """label -> compact record, as `records_of` gives it, out of the file's content"""
    labels = [" + ".join(c) for c in cases_of(function)]
    assert len(labels) == len(data["cases"][function]), "the table does not hold the cases of cases_of()"
    at = data["values"].__getitem__
    return {label: {key: [at(w) for w in v] if key == "warnings" else dict(at(d) for d in v) if key == "binding" else at(v)
                    for key, v in data["records"][place].items()} for label, place in zip(labels, data["cases"][function])}


def dump(data, path):
    """one line per value; records eight and cases forty to the line"""
    js = lambda x: json.dumps(x, sort_keys=True)
    rows = lambda items, per: ",\n   ".join(", ".join(items[i:i + per]) for i in range(0, len(items), per))
    with open(path, "w") as f:
        f.write('{"format": %s,\n "values": [\n   %s],\n' % (js(data["format"]), ",\n   ".join(js(v) for v in data["values"])))
        f.write(' "records": [\n   %s],\n "cases": {\n' % rows([js(r) for r in data["records"]], 8))
        f.write(",\n".join('  %s: [\n   %s]' % (js(fn), rows([str(i) for i in places], 40)) for fn, places in data["cases"].items()))
        f.write("\n }\n}\n")


def main():
    data = encode({function: records_of(function) for function in FUNCTIONS})
    dump(data, OUT)
    print("%d cases, %d distinct records, %d values -> %s" % (sum(len(c) for c in data["cases"].values()), len(data["records"]), len(data["values"]), OUT))


if __name__ == "__main__":
    main()
