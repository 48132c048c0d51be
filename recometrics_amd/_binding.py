"""ctypes binding of include/recometrics_hip.h (the C-ABI of librecometrics_hip.so).

Plays the role of the reference's Cython layer (recometrics/wrapper.pyx:226-495): pulls the raw buffers out of
the NumPy / SciPy objects, pre-allocates the outputs (size 0 == "not requested" == NULL pointer,
wrapper.pyx:208-224,:270-280) and turns status codes into the exceptions `except +` produces there.
There is NO fallback: if the HIP library is missing or there is no device, calls raise.
"""
import ctypes as C
import os

import numpy as np

_LIB_PATH = os.environ.get("RECOMETRICS_HIP_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "csrc", "librecometrics_hip.so")
_lib = None

METRIC_ORDER = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr")
OUTPUTS = tuple(name + ("_auc" if name in ("roc", "pr") else "_at_k") for name in METRIC_ORDER)      # the header's names of the ten outputs

_vp, _i32, _i64, _u64, _sz, _ci = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_int
_FACTORS = (("A", _vp), ("lda", _sz), ("B", _vp), ("ldb", _sz), ("m", _i32), ("n", _i32), ("k", _i32))
_SCORES = (("S", _vp), ("lds", _sz), ("m", _i32), ("n", _i32))


def _csr(which, host, values=False):
    """the CSR arrays `which` (train, test, excl) of an entry; the device form takes the length of the index array too"""
    return ((("X%s_csr_p" % which, _vp), ("X%s_csr_i" % which, _vp)) + ((("X%s_csr" % which, _vp),) if values else ())
            + (() if host else (("nnz_" + which, _i64),)))


def _metrics(source, host):
    return (source + _csr("train", host) + _csr("test", host, values=True) + (("k_metrics", _i32), ("cumulative", _ci))
            + ((("break_ties_with_noise", _ci),) if source is _FACTORS else ()) + tuple((name, _vp) for name in OUTPUTS)
            + (("consider_cold_start", _ci), ("min_items_pool", _i32), ("min_pos_test", _i32)) + ((("nthreads", _i32),) if host else ())
            + ((("seed", _u64),) if source is _FACTORS else ()) + (() if host else (("stream", _vp),)))


def _lists(source, host):
    return (source + _csr("excl", host) + (("k_top", _i32), ("idx", _vp), ("score", _vp), ("status", _vp))
            + ((("nthreads", _i32),) if host else (("stream", _vp),)))


_RANK = (_FACTORS + _csr("train", True) + _csr("test", True)
         + (("k_metrics", _i32), ("break_ties_with_noise", _ci), ("consider_cold_start", _ci), ("min_items_pool", _i32), ("min_pos_test", _i32),
            ("seed", _u64), ("topk_idx", _vp), ("topk_score", _vp), ("pos_rank", _vp), ("status", _vp)))
# one row for the _f32 and the _f64 symbol of a name: the parameters of include/recometrics_hip.h by name, every one returns an int
_TYPED = {"rm_rank": _RANK, "rm_debug_scores": _FACTORS + (("out", _vp),),
          "rm_split": (("X_csr_p", _vp), ("X_csr_i", _vp), ("X_csr", _vp), ("m", _i32), ("n", _i32), ("mode", _ci), ("n_users_test", _i32),
                       ("test_fraction", C.c_double), ("consider_cold_start", _ci), ("min_items_pool", _i32), ("min_pos_test", _i32),
                       ("seed", _u64), ("result", C.POINTER(_vp)))}
_TYPED.update({"rm_" + request + source + form: pieces(params, host) for request, pieces in (("calc_metrics", _metrics), ("recommend", _lists))
               for source, params in (("", _FACTORS), ("_scores", _SCORES)) for form, host in (("", True), ("_dev", False))})
# symbol -> (its (parameter name, ctype) pairs in the header's order, restype)
SIGNATURES = {name + suffix: (params, _ci) for name, params in _TYPED.items() for suffix in ("_f32", "_f64")}
SIGNATURES.update({
    "rm_has_openmp": ((), _ci), "rm_last_error": ((), C.c_char_p), "rm_device_count": ((), _ci), "rm_set_device": ((("device", _ci),), _ci),
    "rm_set_devices": ((("devices", C.POINTER(_i32)), ("n", _i32)), _ci), "rm_get_devices": ((("devices", C.POINTER(_i32)), ("cap", _i32)), _ci),
    "rm_request_interrupt": ((), None), "rm_get_timings": ((("out", C.POINTER(C.c_double)), ("n", _ci)), _ci), "rm_release_workspace": ((), _ci),
    "rm_debug_reload_switches": ((), None), "rm_debug_sweep_variants": ((("elem_bytes", _ci), ("out", C.POINTER(_ci)), ("cap", _ci)), _ci),
    "rm_debug_find_sweep": (tuple((name, _ci) for name in ("elem_bytes", "ng", "ngt", "auc", "dump", "lmode", "nsub", "spec"))
                            + (("out6", C.POINTER(_ci)),), _ci),
    "rm_debug_supported_ng": ((("elem_bytes", _ci), ("k", _ci)), _ci),
    "rm_debug_sweep_launched": ((("elem_bytes", _ci), ("counts", C.POINTER(_ci)), ("cap", _ci)), _ci), "rm_debug_sweep_launched_reset": ((), None),
    "rm_debug_ws_check": ((("msg", C.POINTER(C.c_char)), ("cap", _ci)), _ci),
    "rm_debug_ws_poke": ((("buffer_id", _ci), ("tail", _ci), ("offset", _ci)), _ci),
    "rm_split_size": ((("result", _vp), ("which", _ci)), _i64), "rm_split_copy": ((("result", _vp), ("which", _ci), ("dst", _vp)), _ci),
    "rm_split_free": ((("result", _vp),), None), "rm_split_last_error": ((), C.c_char_p),
    "rm_csr_rows_sorted": ((("indptr", _vp), ("indices", _vp), ("m", _i32), ("nthreads", _i32)), _ci),
    "rm_csr_sort_rows": ((("indptr", _vp), ("indices", _vp), ("values", _vp), ("value_bytes", _i32), ("m", _i32), ("nthreads", _i32)), _ci),
})
EXPORTS = tuple(SIGNATURES)
# include/recometrics_hip_half.h: the four from-scores entries with S in IEEE binary16 ("f16") / bfloat16 ("bf16") bit patterns; every
# other array is the _f32 entry's, so the parameters are the same rows
HALF_KINDS = ("f16", "bf16")
HALF_SIGNATURES = {"rm_" + request + "_scores" + form + "_" + kind: (pieces(_SCORES, host), _ci)
                   for request, pieces in (("calc_metrics", _metrics), ("recommend", _lists)) for form, host in (("", True), ("_dev", False))
                   for kind in HALF_KINDS}
# include/recometrics_hip_half_factors.h: the four factor entries with A and B in 16-bit patterns of one kind; again the _f32 rows
HALF_FACTOR_SIGNATURES = {"rm_" + request + form + "_" + kind: (pieces(_FACTORS, host), _ci)
                          for request, pieces in (("calc_metrics", _metrics), ("recommend", _lists)) for form, host in (("", True), ("_dev", False))
                          for kind in HALF_KINDS}
# test hooks the library exports beside the header's API (csrc/rm_lib.hip states what each is for): same form as SIGNATURES
TEST_HOOKS = {"rm_debug_set_list_ids": ((("ids", C.POINTER(_i32)), ("m", _i32), ("K", _i32)), _ci)}


class HipLibraryMissing(ImportError):
    pass


def lib_path():
    return _LIB_PATH


def _declare(lib, names, table=None):
    """gives the symbols `names` of a loaded library the types SIGNATURES (or `table`) states"""
    for name in names:
        params, restype = (table or SIGNATURES)[name]
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [ctype for _, ctype in params], restype
    return lib


def load():
    """Loads the HIP library (once).  Raises HipLibraryMissing if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise HipLibraryMissing(
                "recometrics_amd: %s is missing -- build it with `python -m recometrics_amd.build` "
                "(there is no CPU fallback)" % _LIB_PATH)
        _lib = _declare(_declare(C.CDLL(_LIB_PATH), SIGNATURES), HALF_SIGNATURES, HALF_SIGNATURES)
        _declare(_lib, HALF_FACTOR_SIGNATURES, HALF_FACTOR_SIGNATURES)
        for name, (params, restype) in TEST_HOOKS.items():      # (a library from before a hook was added loads all the same)
            fn = getattr(_lib, name, None)
            if fn is not None:
                fn.argtypes, fn.restype = [ctype for _, ctype in params], restype
    return _lib


_split_lib = None


def _load_split():
    """The library that provides the host-only rm_split_* and rm_csr_*: librecometrics_hip.so, or -- RECOMETRICS_SPLIT_LIB -- another
    build of csrc/rm_split.cpp and csrc/rm_csr.cpp alone (the sanitizer build of oracle/Makefile, which has no device code to link)."""
    global _split_lib
    alt = os.environ.get("RECOMETRICS_SPLIT_LIB")
    if not alt:
        return load()
    if _split_lib is None:
        _split_lib = _declare(C.CDLL(alt), [name for name in SIGNATURES if name.startswith(("rm_split_", "rm_csr_"))])
    return _split_lib


def _raise(lib, rc):
    msg = (lib.rm_last_error() or b"").decode(errors="replace")
    if rc == 1:
        raise ValueError(msg)
    if rc == 3:
        raise MemoryError(msg)
    if rc == 5:
        # the reference throws std::runtime_error("Error: procedure was interrupted.") after re-raising SIGINT
        # (src/recometrics.hpp:166-173); Cython's `except +` turns it into this RuntimeError, and Python's own handler
        # raises KeyboardInterrupt for the re-raised signal
        raise RuntimeError(msg.strip())
    raise RuntimeError("recometrics_amd (status %d): %s" % (rc, msg))


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def _dp(x):
    """an integer device address (0 == NULL)"""
    return C.c_void_p(int(x)) if x else None


def _metric_outs(outs, want, m, k_metrics, cumulative, dtype):
    """The ten outputs of a host entry in METRIC_ORDER, as the reference's cpp_funs.calc_reco_metrics returns them (wrapper.pyx:306-323):
    size-0 arrays for metrics not requested, (m, k) arrays for cumulative top-K metrics.  `outs`: ten caller-owned flat arrays
    (size 0 = not requested) instead of new ones."""
    if outs is None:
        size_arr = m * k_metrics if cumulative else m
        outs = [np.empty((m if name in ("roc", "pr") else size_arr) if want.get(name) else 0, dtype=dtype) for name in METRIC_ORDER]
    if cumulative:
        outs = [(o.reshape((m, k_metrics)) if o.size else o.reshape((0, 0))) if i < 8 else o for i, o in enumerate(outs)]
    return tuple(outs)


def _list_outs(m, k_top, dtype, return_scores=True):
    """ids [m, k_top], scores [m, k_top] or None, status [m] of a list entry"""
    return (np.empty((m, k_top), dtype=np.int32), np.empty((m, k_top), dtype=dtype) if return_scores else None, np.empty(m, dtype=np.int32))


def has_openmp():
    return bool(load().rm_has_openmp())


def device_count():
    return int(load().rm_device_count())


def set_device(i):
    lib = load()
    rc = lib.rm_set_device(int(i))
    if rc:
        _raise(lib, rc)


def set_devices(devices):
    """Devices of the host-pointer calls of this process (rm_set_devices): a list of device ids, the same id may repeat;
    an empty list restores "the current device"."""
    lib = load()
    arr = (C.c_int32 * max(len(devices), 1))(*devices)
    rc = lib.rm_set_devices(arr, len(devices))
    if rc:
        _raise(lib, rc)


def get_devices():
    lib = load()
    buf = (C.c_int32 * 64)()
    n = lib.rm_get_devices(buf, 64)
    return [int(buf[i]) for i in range(min(n, 64))]


def request_interrupt():
    load().rm_request_interrupt()


def reload_switches():
    """Test hook: the library reads its RM_DEBUG_* switches from the environment when it is loaded; this reads them again."""
    load().rm_debug_reload_switches()


def timings():
    lib = load()
    buf = (C.c_double * 11)()
    n = lib.rm_get_timings(buf, 11)
    keys = ("prep_ms", "sweep_ms", "finalize_ms", "device_ms", "sweep_launches", "item_splits", "sweep_blocks", "lds_bytes",
            "timed_slots", "total_slots", "split_reused")
    return {k: buf[i] for i, k in enumerate(keys[:n])}


def hinted_users():
    """Users whose top-K bound the most recent pass seeded from the lists the call before it left on the kept split (slot 12 of
    rm_get_timings; 0 when the pass had no such lists, or a library from before there were any)."""
    lib = load()
    buf = (C.c_double * 12)()
    return int(buf[11]) if lib.rm_get_timings(buf, 12) >= 12 else 0


def set_list_ids(ids):
    """Test hook (rm_debug_set_list_ids): overwrites the item ids of the lists the context keeps for its next pass with `ids` [m, K]."""
    lib = load()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    rc = lib.rm_debug_set_list_ids(ids.ctypes.data_as(C.POINTER(_i32)), ids.shape[0], ids.shape[1])
    if rc:
        _raise(lib, rc)


def ws_check():
    """Test hook (rm_debug_ws_check) of RM_DEBUG_WS_GUARD: (damaged zones, buffers checked, the report's text) of the current device's
    workspace buffers."""
    lib = load()
    buf = C.create_string_buffer(1 << 16)
    damaged = lib.rm_debug_ws_check(buf, len(buf))
    if damaged < 0:
        _raise(lib, 2)
    text = buf.value.decode()
    return damaged, int(text.split()[1]), text


def ws_poke(buffer_id, tail, offset):
    """Test hook (rm_debug_ws_poke): damages one byte of a red zone of the live guarded buffer `buffer_id`."""
    lib = load()
    rc = lib.rm_debug_ws_poke(int(buffer_id), int(bool(tail)), int(offset))
    if rc:
        _raise(lib, rc)


def csr_rows_sorted(indptr, indices, nthreads=0):
    """True when the column indices of every row of an int32 CSR ascend (rm_csr_rows_sorted: multi-threaded pass)."""
    lib = _load_split()
    assert indptr.dtype == np.int32 and indices.dtype == np.int32
    rc = lib.rm_csr_rows_sorted(_p(indptr), _p(indices), indptr.shape[0] - 1, int(nthreads))
    if rc < 0:
        raise ValueError("rm_csr_rows_sorted: bad argument")
    return bool(rc)


def csr_sort_rows(indptr, indices, data, nthreads=0):
    """Sorts every row's (index, value) pairs by index, in place (rm_csr_sort_rows); `data` may be None."""
    lib = _load_split()
    assert indptr.dtype == np.int32 and indices.dtype == np.int32 and indices.flags.writeable
    vb = 0 if data is None else data.dtype.itemsize
    if vb not in (0, 4, 8):
        raise ValueError("values must be 4 or 8 bytes wide")
    rc = lib.rm_csr_sort_rows(_p(indptr), _p(indices), None if data is None else _p(data), vb, indptr.shape[0] - 1, int(nthreads))
    if rc:
        raise (MemoryError if rc == 3 else ValueError)("rm_csr_sort_rows failed (status %d)" % rc)


def _invoke(entry, dtype, **values):
    """Calls `entry`'s symbol for `dtype` (or, "f16" / "bf16", its symbol of HALF_SIGNATURES / HALF_FACTOR_SIGNATURES) with `values` given by the header's
    parameter names, in the order SIGNATURES states; a status other than 0 raises (`_raise`).  A missing name is a KeyError and an unknown one a TypeError, both before the call."""
    if dtype in HALF_KINDS:
        name = entry + "_" + dtype
        params = (HALF_SIGNATURES if name in HALF_SIGNATURES else HALF_FACTOR_SIGNATURES)[name][0]
    else:
        name = entry + ("_f32" if dtype == np.float32 else "_f64")
        params = SIGNATURES[name][0]
    args = [values[param] for param, _ in params]
    if len(values) != len(params):
        raise TypeError("%s has no parameter %s" % (name, ", ".join(sorted(set(values) - {param for param, _ in params}))))
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc:
        _raise(lib, rc)


def _metrics_values(ptr, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test):
    """what the four metric entries share, by name; `ptr`: `_p` for host arrays, `_dp` for device addresses"""
    return dict(zip(OUTPUTS, map(ptr, outs)), Xtrain_csr_p=ptr(train_p), Xtrain_csr_i=ptr(train_i), Xtest_csr_p=ptr(test_p), Xtest_csr_i=ptr(test_i),
                Xtest_csr=ptr(test_v), k_metrics=k_metrics, cumulative=int(bool(cumulative)), consider_cold_start=int(bool(consider_cold_start)),
                min_items_pool=min_items_pool, min_pos_test=min_pos_test)


def _host_excl_p(excl_p):
    """None: nothing is left out; an array goes over as it is, also an empty one (`_p` would make that NULL)"""
    return None if excl_p is None else excl_p.ctypes.data_as(C.c_void_p)


def calc_metrics(A, lda, B, ldb, train_p, train_i, test_p, test_i, test_v, k_metrics, want, cumulative,
                 break_ties_with_noise, consider_cold_start, min_items_pool, min_pos_test, nthreads, seed, outs=None):
    """Host-array entry.  `want`: dict metric-name -> bool in METRIC_ORDER.  Returns the 10-tuple of arrays the
    reference's cpp_funs.calc_reco_metrics returns (wrapper.pyx:306-323): size-0 arrays for metrics not requested,
    (m, k) arrays for cumulative top-K metrics."""
    dtype = A.dtype.type
    m, k = A.shape
    outs = _metric_outs(outs, want, m, k_metrics, cumulative, dtype)
    _invoke("rm_calc_metrics", dtype, A=_p(A), lda=lda, B=_p(B), ldb=ldb, m=m, n=B.shape[0], k=k,
            break_ties_with_noise=int(bool(break_ties_with_noise)), nthreads=nthreads, seed=seed,
            **_metrics_values(_p, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))
    return outs


def calc_metrics_device(dtype, A, lda, B, ldb, m, n, k, train_p, train_i, nnz_train, test_p, test_i, test_v, nnz_test,
                        k_metrics, outs, cumulative=False, break_ties_with_noise=False, consider_cold_start=True,
                        min_items_pool=2, min_pos_test=1, seed=1, stream=0):
    """Device-pointer entry: every array argument is an integer device address (0 == NULL); `outs` is a sequence
    of 10 addresses in METRIC_ORDER.  Asynchronous on `stream` apart from one small plan read-back."""
    _invoke("rm_calc_metrics_dev", dtype, A=_dp(A), lda=lda, B=_dp(B), ldb=ldb, m=m, n=n, k=k, nnz_train=nnz_train, nnz_test=nnz_test,
            break_ties_with_noise=int(bool(break_ties_with_noise)), seed=seed, stream=_dp(stream),
            **_metrics_values(_dp, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))


def calc_metrics_scores(S, lds, train_p, train_i, test_p, test_i, test_v, k_metrics, want, cumulative,
                        consider_cold_start, min_items_pool, min_pos_test, nthreads, outs=None):
    """Host-array entry of the metrics from a score matrix (rm_calc_metrics_scores_*): `S` [m, n] row-major with leading
    dimension `lds` (elements), the rest as `calc_metrics` without tie noise and seed.  Returns the same 10-tuple."""
    dtype = S.dtype.type
    m, n = S.shape
    outs = _metric_outs(outs, want, m, k_metrics, cumulative, dtype)
    _invoke("rm_calc_metrics_scores", dtype, S=_p(S), lds=lds, m=m, n=n, nthreads=nthreads,
            **_metrics_values(_p, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))
    return outs


def calc_metrics_scores_device(dtype, S, lds, m, n, train_p, train_i, nnz_train, test_p, test_i, test_v, nnz_test,
                               k_metrics, outs, cumulative=False, consider_cold_start=True,
                               min_items_pool=2, min_pos_test=1, stream=0):
    """Device-pointer entry (rm_calc_metrics_scores_dev_*): every array argument is an integer device address (0 == NULL);
    `outs` is a sequence of 10 addresses in METRIC_ORDER.  Asynchronous on `stream` apart from one small plan read-back."""
    _invoke("rm_calc_metrics_scores_dev", dtype, S=_dp(S), lds=lds, m=m, n=n, nnz_train=nnz_train, nnz_test=nnz_test, stream=_dp(stream),
            **_metrics_values(_dp, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))


def half_kind(S):
    """"f16" for a float16 array, "bf16" for a uint16 one (bfloat16 bit patterns: NumPy has no such dtype)"""
    if S.dtype == np.float16:
        return "f16"
    if S.dtype == np.uint16:
        return "bf16"
    raise TypeError("16-bit scores are a float16 array, or bfloat16 bit patterns as uint16 (got %s)" % S.dtype)


def calc_metrics_scores_half(S, lds, train_p, train_i, test_p, test_i, test_v, k_metrics, want, cumulative,
                             consider_cold_start, min_items_pool, min_pos_test, nthreads, outs=None):
    """`calc_metrics_scores` for 16-bit scores (rm_calc_metrics_scores_f16 / _bf16): `S` [m, n] a float16 array, or bfloat16 bit
    patterns as uint16, with leading dimension `lds` in 2-byte elements; `test_v` and the ten outputs are float32."""
    m, n = S.shape
    outs = _metric_outs(outs, want, m, k_metrics, cumulative, np.float32)
    _invoke("rm_calc_metrics_scores", half_kind(S), S=_p(S), lds=lds, m=m, n=n, nthreads=nthreads,
            **_metrics_values(_p, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))
    return outs


def calc_metrics_scores_half_device(kind, S, lds, m, n, train_p, train_i, nnz_train, test_p, test_i, test_v, nnz_test,
                                    k_metrics, outs, cumulative=False, consider_cold_start=True,
                                    min_items_pool=2, min_pos_test=1, stream=0):
    """`calc_metrics_scores_device` for 16-bit scores: `kind` "f16" / "bf16" in the place of the dtype, everything else float32"""
    assert kind in HALF_KINDS
    _invoke("rm_calc_metrics_scores_dev", kind, S=_dp(S), lds=lds, m=m, n=n, nnz_train=nnz_train, nnz_test=nnz_test, stream=_dp(stream),
            **_metrics_values(_dp, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))


def recommend_scores_half(S, lds, excl_p, excl_i, k_top, return_scores=True, nthreads=0):
    """`recommend_scores` for 16-bit scores (rm_recommend_scores_f16 / _bf16): `S` as in `calc_metrics_scores_half`; the list scores
    are float32."""
    m, n = S.shape
    idx, sc, st = _list_outs(m, k_top, np.float32, return_scores)
    _invoke("rm_recommend_scores", half_kind(S), S=_p(S), lds=lds, m=m, n=n, Xexcl_csr_p=_host_excl_p(excl_p), Xexcl_csr_i=_p(excl_i),
            k_top=k_top, idx=_p(idx), score=_p(sc), status=_p(st), nthreads=int(nthreads))
    return idx, sc, st


def recommend_scores_half_device(kind, S, lds, m, n, excl_p, excl_i, nnz_excl, k_top, idx, score, status, stream=0):
    """`recommend_scores_device` for 16-bit scores: `kind` "f16" / "bf16" in the place of the dtype, `score` float32"""
    assert kind in HALF_KINDS
    _invoke("rm_recommend_scores_dev", kind, S=_dp(S), lds=lds, m=m, n=n, Xexcl_csr_p=_dp(excl_p), Xexcl_csr_i=_dp(excl_i),
            nnz_excl=nnz_excl, k_top=k_top, idx=_dp(idx), score=_dp(score), status=_dp(status), stream=_dp(stream))


def calc_metrics_half(A, lda, B, ldb, train_p, train_i, test_p, test_i, test_v, k_metrics, want, cumulative,
                      break_ties_with_noise, consider_cold_start, min_items_pool, min_pos_test, nthreads, seed, outs=None):
    """`calc_metrics` for 16-bit factors (rm_calc_metrics_f16 / _bf16): `A` [m, k] and `B` [n, k] float16 arrays, or bfloat16 bit
    patterns as uint16, both of one kind, with leading dimensions in 2-byte elements; `test_v` and the ten outputs are float32."""
    kind = half_kind(A)
    if half_kind(B) != kind:
        raise TypeError("A and B must hold the same 16-bit type")
    m, k = A.shape
    outs = _metric_outs(outs, want, m, k_metrics, cumulative, np.float32)
    _invoke("rm_calc_metrics", kind, A=_p(A), lda=lda, B=_p(B), ldb=ldb, m=m, n=B.shape[0], k=k,
            break_ties_with_noise=int(bool(break_ties_with_noise)), nthreads=nthreads, seed=seed,
            **_metrics_values(_p, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))
    return outs


def calc_metrics_half_device(kind, A, lda, B, ldb, m, n, k, train_p, train_i, nnz_train, test_p, test_i, test_v, nnz_test,
                             k_metrics, outs, cumulative=False, break_ties_with_noise=False, consider_cold_start=True,
                             min_items_pool=2, min_pos_test=1, seed=1, stream=0):
    """`calc_metrics_device` for 16-bit factors: `kind` "f16" / "bf16" in the place of the dtype, everything else float32"""
    assert kind in HALF_KINDS
    _invoke("rm_calc_metrics_dev", kind, A=_dp(A), lda=lda, B=_dp(B), ldb=ldb, m=m, n=n, k=k, nnz_train=nnz_train, nnz_test=nnz_test,
            break_ties_with_noise=int(bool(break_ties_with_noise)), seed=seed, stream=_dp(stream),
            **_metrics_values(_dp, train_p, train_i, test_p, test_i, test_v, k_metrics, cumulative, outs, consider_cold_start, min_items_pool, min_pos_test))


def recommend_half(A, lda, B, ldb, excl_p, excl_i, k_top, return_scores=True, nthreads=0):
    """`recommend` for 16-bit factors (rm_recommend_f16 / _bf16): `A`, `B` as in `calc_metrics_half`; the list scores are float32."""
    kind = half_kind(A)
    if half_kind(B) != kind:
        raise TypeError("A and B must hold the same 16-bit type")
    m, k = A.shape
    idx, sc, st = _list_outs(m, k_top, np.float32, return_scores)
    _invoke("rm_recommend", kind, A=_p(A), lda=lda, B=_p(B), ldb=ldb, m=m, n=B.shape[0], k=k, Xexcl_csr_p=_host_excl_p(excl_p), Xexcl_csr_i=_p(excl_i),
            k_top=k_top, idx=_p(idx), score=_p(sc), status=_p(st), nthreads=int(nthreads))
    return idx, sc, st


def recommend_half_device(kind, A, lda, B, ldb, m, n, k, excl_p, excl_i, nnz_excl, k_top, idx, score, status, stream=0):
    """`recommend_device` for 16-bit factors: `kind` "f16" / "bf16" in the place of the dtype, `score` float32"""
    assert kind in HALF_KINDS
    _invoke("rm_recommend_dev", kind, A=_dp(A), lda=lda, B=_dp(B), ldb=ldb, m=m, n=n, k=k, Xexcl_csr_p=_dp(excl_p), Xexcl_csr_i=_dp(excl_i),
            nnz_excl=nnz_excl, k_top=k_top, idx=_dp(idx), score=_dp(score), status=_dp(status), stream=_dp(stream))


def rank(A, B, train_p, train_i, test_p, test_i, k_metrics, break_ties_with_noise=False, consider_cold_start=True,
         min_items_pool=2, min_pos_test=1, seed=1):
    dtype = A.dtype.type
    m, k = A.shape
    idx, sc, st = _list_outs(m, k_metrics, dtype)
    pr = np.zeros(max(int(test_i.shape[0]), 1), dtype=np.int64)
    A = np.ascontiguousarray(A)                  # the raw pointer is passed with lda = k: rows must be dense
    B = np.ascontiguousarray(B)
    _invoke("rm_rank", dtype, A=_p(A), lda=A.shape[1], B=_p(B), ldb=B.shape[1], m=m, n=B.shape[0], k=k,
            Xtrain_csr_p=_p(train_p), Xtrain_csr_i=_p(train_i), Xtest_csr_p=_p(test_p), Xtest_csr_i=_p(test_i), k_metrics=k_metrics,
            break_ties_with_noise=int(bool(break_ties_with_noise)), consider_cold_start=int(bool(consider_cold_start)),
            min_items_pool=min_items_pool, min_pos_test=min_pos_test, seed=seed, topk_idx=_p(idx), topk_score=_p(sc), pos_rank=_p(pr), status=_p(st))
    return {"topk_idx": idx, "topk_score": sc, "pos_rank": pr[:test_i.shape[0]], "status": st}


def recommend(A, lda, B, ldb, excl_p, excl_i, k_top, return_scores=True, nthreads=0):
    """Host-array entry of the recommendation lists (rm_recommend_*): A [m, k] / B [n, k] row-major with leading dimensions
    lda / ldb, `excl_p` / `excl_i` the int32 CSR of the items to leave out per user (`excl_p` None: nothing is left out).
    Returns (ids [m, k_top] int32, scores [m, k_top] or None, status [m] int32); -1 / NaN where a row holds no entry."""
    dtype = A.dtype.type
    m, k = A.shape
    idx, sc, st = _list_outs(m, k_top, dtype, return_scores)
    _invoke("rm_recommend", dtype, A=_p(A), lda=lda, B=_p(B), ldb=ldb, m=m, n=B.shape[0], k=k, Xexcl_csr_p=_host_excl_p(excl_p), Xexcl_csr_i=_p(excl_i),
            k_top=k_top, idx=_p(idx), score=_p(sc), status=_p(st), nthreads=int(nthreads))
    return idx, sc, st


def recommend_device(dtype, A, lda, B, ldb, m, n, k, excl_p, excl_i, nnz_excl, k_top, idx, score, status, stream=0):
    """Device-pointer entry (rm_recommend_dev_*): every array argument is an integer device address (0 == NULL: `excl_p` = nothing
    is left out, `score` = ids only).  Asynchronous on `stream` apart from one small plan read-back."""
    _invoke("rm_recommend_dev", dtype, A=_dp(A), lda=lda, B=_dp(B), ldb=ldb, m=m, n=n, k=k, Xexcl_csr_p=_dp(excl_p), Xexcl_csr_i=_dp(excl_i),
            nnz_excl=nnz_excl, k_top=k_top, idx=_dp(idx), score=_dp(score), status=_dp(status), stream=_dp(stream))


def recommend_scores(S, lds, excl_p, excl_i, k_top, return_scores=True, nthreads=0):
    """Host-array entry of the recommendation lists from a score matrix (rm_recommend_scores_*): `S` [m, n] row-major with leading
    dimension `lds` (elements), the rest and the return value as `recommend`."""
    dtype = S.dtype.type
    m, n = S.shape
    idx, sc, st = _list_outs(m, k_top, dtype, return_scores)
    _invoke("rm_recommend_scores", dtype, S=_p(S), lds=lds, m=m, n=n, Xexcl_csr_p=_host_excl_p(excl_p), Xexcl_csr_i=_p(excl_i),
            k_top=k_top, idx=_p(idx), score=_p(sc), status=_p(st), nthreads=int(nthreads))
    return idx, sc, st


def recommend_scores_device(dtype, S, lds, m, n, excl_p, excl_i, nnz_excl, k_top, idx, score, status, stream=0):
    """Device-pointer entry (rm_recommend_scores_dev_*): every array argument is an integer device address (0 == NULL: `excl_p` =
    nothing is left out, `score` = ids only).  Asynchronous on `stream` apart from one small plan read-back."""
    _invoke("rm_recommend_scores_dev", dtype, S=_dp(S), lds=lds, m=m, n=n, Xexcl_csr_p=_dp(excl_p), Xexcl_csr_i=_dp(excl_i),
            nnz_excl=nnz_excl, k_top=k_top, idx=_dp(idx), score=_dp(score), status=_dp(status), stream=_dp(stream))


def debug_scores(A, B):
    dtype = A.dtype.type
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    out = np.empty((A.shape[0], B.shape[0]), dtype=dtype)
    _invoke("rm_debug_scores", dtype, A=_p(A), lda=A.shape[1], B=_p(B), ldb=B.shape[1], m=A.shape[0], n=B.shape[0], k=A.shape[1], out=_p(out))
    return out


def split_csr(indptr, indices, data, n_items, mode, n_users_test=0, test_fraction=0.3, consider_cold_start=False,
              min_items_pool=2, min_pos_test=1, seed=1):
    """Host-side split (rm_split_*): returns a dict of raw arrays -- "train" / "test" / "rem" as (indptr, indices, data)
    tuples and "users_test".  mode: 0 every row, 1 separated, 2 joined (reference wrapper.pyx:523-818)."""
    lib = _load_split()
    dtype = data.dtype.type
    fn = lib.rm_split_f32 if dtype == np.float32 else lib.rm_split_f64
    handle = C.c_void_p()
    m = indptr.shape[0] - 1
    rc = fn(_p(indptr), _p(indices), _p(data), m, n_items, mode, n_users_test, float(test_fraction),
            int(bool(consider_cold_start)), min_items_pool, min_pos_test, seed, C.byref(handle))
    if rc:
        msg = (lib.rm_split_last_error() or b"").decode(errors="replace")
        if rc == 3:
            raise MemoryError(msg)
        raise RuntimeError(msg)
    try:
        def arr(which, dt):
            cnt = lib.rm_split_size(handle, which)
            out = np.empty(max(cnt, 0), dtype=dt)
            if cnt > 0:
                lib.rm_split_copy(handle, which, out.ctypes.data_as(C.c_void_p))
            return out
        res = {}
        for name, base in (("train", 0), ("test", 3), ("rem", 6)):
            res[name] = (arr(base, np.int32), arr(base + 1, np.int32), arr(base + 2, dtype))
        res["users_test"] = arr(9, np.int32)
        return res
    finally:
        lib.rm_split_free(handle)
