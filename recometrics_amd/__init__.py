"""recometrics_amd -- MI355X-native drop-in for the ranking-metric hot path of david-cortes/recometrics.

Public surface = the reference's ``calc_reco_metrics`` (recometrics/__init__.py:44-628): same keyword arguments,
defaults, error / warning conditions, dtype rule and output naming.  The per-user work (score the item pool, mask
train items, top-K, P/TP/R/AP/TAP/NDCG/Hit/RR@K, ROC/PR-AUC) runs in hand-written HIP kernels behind the C-ABI of
``include/recometrics_hip.h``.  There is no CPU fallback: without the built library and a GPU the call raises.
"""
import multiprocessing
from warnings import warn

import numpy as np

from . import _binding

__all__ = ["calc_reco_metrics", "calc_reco_metrics_from_scores", "recommend_topk", "recommend_topk_from_scores", "split_reco_train_test"]
__version__ = "0.1.0"

# (keyword of calc_reco_metrics, name in the C-ABI order, key of the result dict) -- reference __init__.py:590-613
_METRICS = (
    ("precision", "p", "P@K"), ("trunc_precision", "tp", "TP@K"), ("recall", "r", "R@K"),
    ("average_precision", "ap", "AP@K"), ("trunc_average_precision", "tap", "TAP@K"), ("ndcg", "ndcg", "NDCG@K"),
    ("hit", "hit", "Hit@K"), ("rr", "rr", "RR@K"), ("roc_auc", "roc", "ROC_AUC"), ("pr_auc", "pr", "PR_AUC"),
)
_INT32_MAX = np.iinfo(np.int32).max


def split_reco_train_test(*args, **kwargs):
    """See :func:`recometrics_amd.split.split_reco_train_test` (imported lazily: it needs SciPy)."""
    from .split import split_reco_train_test as impl
    return impl(*args, **kwargs)


def _row_major_with_ld(X):
    """(array, leading dimension in elements): a row-major view keeps its stride, anything else is copied
    (reference __init__.py:11-16)."""
    if X.flags["C_CONTIGUOUS"]:
        return X, X.shape[1]
    st0 = X.strides[0]
    if X.strides[1] == X.dtype.itemsize and st0 > 0 and st0 % X.itemsize == 0 and st0 // X.itemsize >= X.shape[1]:
        return X, st0 // X.itemsize
    return np.ascontiguousarray(X), X.shape[1]          # reversed / overlapping / unaligned rows: a size_t cannot express them


def _csr_int32(X):
    """CSR with int32 index arrays over contiguous buffers (reference __init__.py:26-41), rows AS THEY ARE.

    The reference sorts the column indices of every row with SciPy's `sort_indices()` -- one thread walking every stored entry
    whenever SciPy does not already know the answer, 26-33 ms for the two matrices of BASELINE C2 in front of a 10 ms device
    call.  Here the rows go to the library as they come: it validates them on the device (sorted? every index in range? index
    pointers monotone?  csrc/rm_prep.hpp k_check_csr_*, ~40 us) and only when some row is not sorted does it sort a COPY on
    the host (csrc/rm_csr.cpp) and run again.  Unlike the reference, the caller's matrix is never modified."""
    from scipy.sparse import csr_array, issparse
    X = X.tocsr() if issparse(X) and X.format != "csr" else (X if issparse(X) else csr_array(X))
    if X.indptr.dtype != np.int32 or X.indices.dtype != np.int32:
        X = csr_array((X.data, X.indices.astype(np.int32), X.indptr.astype(np.int32)), shape=X.shape, copy=False)
    return X


def _sorted_csr_int32(X, nthreads=0):
    """CSR with sorted column indices and int32 index arrays (reference __init__.py:26-41), for the HOST-side split
    (split.py: its C++ walks the rows on the CPU and must see what the reference sees).

    A matrix whose index arrays are int32 already is sorted in place, like the reference does; one with int64 indices is
    copied first (the reference sorts the caller's matrix, then copies).  SciPy's cached answer (`_has_sorted_indices`, the
    attribute behind the public `has_sorted_indices` property, whose getter runs SciPy's single-threaded check when the answer
    is unknown) is trusted when it says True; tests/test_csr_cpu.py pins the attribute's name for the installed SciPy --
    should a release rename it, every call merely pays for the library's check again.  Otherwise the check -- and the sort,
    should it be needed -- run in the library on `nthreads` host threads (csrc/rm_csr.cpp) and the flag is set."""
    from scipy.sparse import csr_array, issparse
    X = X.tocsr() if issparse(X) and X.format != "csr" else (X if issparse(X) else csr_array(X))
    if X.indptr.dtype != np.int32 or X.indices.dtype != np.int32:
        known = getattr(X, "_has_sorted_indices", None)
        X = X.copy()
        X.indptr, X.indices = X.indptr.astype(np.int32), X.indices.astype(np.int32)
        if known:
            X.has_sorted_indices = True
    if getattr(X, "_has_sorted_indices", None) is True:       # SciPy's cached answer (set by its own sort / check, or by us below)
        return X
    if not (X.indices.flags.c_contiguous and X.indptr.flags.c_contiguous and X.data.flags.c_contiguous
            and X.data.dtype.itemsize in (4, 8) and X.indices.flags.writeable and X.data.flags.writeable):
        X.sort_indices()                                        # unusual storage: SciPy's own pass
        return X
    if not _binding.csr_rows_sorted(X.indptr, X.indices, nthreads):
        _binding.csr_sort_rows(X.indptr, X.indices, X.data, nthreads)
    X.has_sorted_indices = True
    return X


def _fail_if(cond, message):
    if cond:
        raise ValueError(message)


def _check_factors(A, B, n_users, n_items):
    """Shape rules of reference __init__.py:442-467; returns A, B trimmed to the test matrix (with its warnings)."""
    _fail_if(A.ndim != 2, "'A' must be a 2-dimensional array.")
    _fail_if(B.ndim != 2, "'B' must be a 2-dimensional array.")
    _fail_if(A.shape[1] != B.shape[1], "'A' and 'B' must have the same number of columns.")
    _fail_if(0 in (A.shape[0], A.shape[1], B.shape[1], n_users, n_items), "Input matrices cannot be empty.")
    _fail_if(A.shape[0] < n_users, "Number of users in 'A' and 'X_test' does not match.")
    _fail_if(B.shape[0] < n_items, "Number of items in 'B' and 'X_test' does not match.")
    if A.shape[0] > n_users:
        warn("'A' has more users than 'X_test'.")
        A = A[:n_users]
    if B.shape[0] > n_items:
        warn("'B' has more items than 'X_test'.")
        B = B[:n_items]
    return A, B


def _fold_item_biases(A, B, item_biases, n_items, dtype):
    """scores = A @ B.T + bias  ==  [A | 1] @ [B | bias].T   (reference __init__.py:534-551)"""
    assert isinstance(item_biases, np.ndarray)
    _fail_if(item_biases.ndim > 2, "'item_biases' should be a 1-d array.")
    item_biases = item_biases.reshape(-1)
    _fail_if(item_biases.shape[0] == 0, "'item_biases' is empty.")
    _fail_if(item_biases.shape[0] < n_items, "Number of items in 'item_biases' must match with 'X_test'.")
    if item_biases.shape[0] > n_items:
        warn("'item_biases' has more items than 'X_test'.")
        item_biases = item_biases[:n_items]
    ones = np.ones((A.shape[0], 1), dtype=dtype)
    return np.hstack([A.astype(dtype, copy=False), ones]), np.hstack([B.astype(dtype, copy=False), item_biases.astype(dtype).reshape(-1, 1)])


def _as_frame(out, k, cumulative, rename_k):
    """dict of arrays -> DataFrame with the reference's column names (__init__.py:615-626): "P@K" -> "P@5", cumulative
    blocks -> "P@1" .. "P@k".  ROC_AUC / PR_AUC stay single columns in cumulative mode (the reference raises there)."""
    import pandas as pd
    if not cumulative:
        df = pd.DataFrame(out)
        if rename_k:
            df.columns = [c[:-1] + str(k) if c.endswith("@K") else c for c in df.columns]
        return df
    blocks = []
    for key, arr in out.items():
        if arr.ndim == 1:
            blocks.append(pd.DataFrame({key: arr}))
        else:
            blocks.append(pd.DataFrame(arr, columns=["%s%d" % (key[:-1], i + 1) for i in range(arr.shape[1])]))
    return pd.concat(blocks, axis=1)


def _requested_metrics(arguments):
    """keyword -> bool out of a metric call's arguments (its `locals()`): the flag, or `all_metrics`"""
    return {name: bool(arguments["all_metrics"] or arguments[name]) for name, _, _ in _METRICS}


def _fail_if_no_ranking_metric(requested):
    _fail_if(not (requested["precision"] or requested["average_precision"] or requested["ndcg"]
                  or requested["hit"] or requested["rr"] or requested["roc_auc"]),
             "Must pass at least one metric to calculate.")


def _train_or_empty(X_train, X_test, dtype, consider_cold_start):
    """(X_train, consider_cold_start): no train matrix is an empty one with cold start on"""
    if X_train is not None:
        return X_train, consider_cold_start
    from scipy.sparse import csr_array
    return csr_array(X_test.shape, dtype=dtype), True


def _split_arrays(X_train, X_test, n_users, dtype):
    """(train_p, train_i, test_p, test_i, test_v) for the binding: int32 CSR (the library validates and, if need be, sorts the rows),
    a taller `X_train` trimmed to the test users, test values in `dtype`; nothing is copied that already has the right type and layout"""
    X_train = _csr_int32(X_train)
    if X_train.shape[0] > n_users:
        X_train = _csr_int32(X_train[:n_users])
    X_test = _csr_int32(X_test)
    test_values = X_test.data if X_test.data.dtype == dtype else X_test.data.astype(dtype)
    return tuple(np.ascontiguousarray(a) for a in (X_train.indptr, X_train.indices, X_test.indptr, X_test.indices, test_values))


def _output_storage(requested, n_users, dtype, as_df, cumulative):
    """(want, outs, block, keys) of a metric call.  For a plain DataFrame the storage is allocated up front: one column-major [users,
    metrics] block whose columns ARE the output arrays of the call -- pandas wraps it without a copy (building the frame from ten
    separate arrays consolidates them into such a block: 0.9 ms for BASELINE C2's 138k users, 8 % of the call)"""
    want = {short: requested[name] for name, short, _ in _METRICS}
    if not as_df or cumulative:
        return want, None, None, None
    keys = [key for (name, _, key) in _METRICS if requested[name]]
    block = np.empty((n_users, len(keys)), dtype=dtype, order="F")
    cols = iter(range(len(keys)))
    return want, [block[:, next(cols)] if requested[name] else np.empty(0, dtype=dtype) for name, _, _ in _METRICS], block, keys


def _metrics_result(arrays, block, keys, k, as_df, cumulative, rename_k):
    """the block's frame, the dict with "K", or the frame of the dict"""
    if block is not None:
        import pandas as pd
        if rename_k:
            keys = [key[:-1] + str(k) if key.endswith("@K") else key for key in keys]
        return pd.DataFrame(block, columns=keys, copy=False)
    out = {key: arr for (_, _, key), arr in zip(_METRICS, arrays) if arr.shape[0]}
    if not as_df:
        out["K"] = k
        return out
    return _as_frame(out, k, bool(cumulative), bool(rename_k))


def _list_length(k, n_items):
    k = int(k)
    _fail_if(k < 1, "'k' must be positive.")
    _fail_if(k > n_items, "'k' should be smaller than the number of items.")
    return k


def _user_selection(users, n_users, source):
    """`users` as an int64 array (or None); `source`: the argument whose rows it selects, for the message"""
    if users is None:
        return None
    users = np.asarray(users)
    _fail_if(users.ndim != 1 or (users.size and users.dtype.kind not in "iu"), "'users' must be a 1-d integer array.")
    users = users.astype(np.int64, copy=False)
    _fail_if(users.size and (users.min() < 0 or users.max() >= n_users), "'users' has entries outside the rows of '%s'." % source)
    return users


def _exclusion_csr(X_train, users):
    """(excl_p, excl_i): the int32 CSR of the items to leave out, its rows gathered by `users`; (None, None) leaves nothing out"""
    if X_train is None:
        return None, None
    if users is not None:
        X_train = _csr_int32(X_train)[users]
    X_train = _csr_int32(X_train)
    return np.ascontiguousarray(X_train.indptr), np.ascontiguousarray(X_train.indices)


def _no_lists(k, dtype, return_scores):
    """the answer for no users at all"""
    return (np.empty((0, k), np.int32), np.empty((0, k), dtype) if return_scores else None, np.empty(0, np.int32))


# ---- `scores` as a torch.Tensor (the from-scores functions) ---------------------------------------------------------------------
def _torch_if_tensor(scores):
    """the torch module when `scores` is a torch.Tensor, else None -- torch is never imported for it: a tensor cannot exist without"""
    import sys
    torch = sys.modules.get("torch")
    return torch if torch is not None and isinstance(scores, torch.Tensor) else None


def _tensor_kind(torch, scores):
    """"f16" / "bf16" (include/recometrics_hip_half.h), np.float32 / np.float64 (the entries NumPy arrays take), None for any other dtype"""
    return {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: np.float32, torch.float64: np.float64}.get(scores.dtype)


def _cpu_tensor_as_array(torch, scores, kind):
    """A CPU tensor as a NumPy array over the SAME memory: float16 / float32 / float64 as they are, bfloat16 -- NumPy has no such dtype
    -- as its bit patterns in uint16.  Strides are kept; `_row_major_with_ld` then passes `stride(1) == 1` with its row stride and
    copies anything else once."""
    scores = scores.detach()
    return scores.view(torch.int16).numpy().view(np.uint16) if kind == "bf16" else scores.numpy()


def _factor_tensors(A, B):
    """(torch, kind) when `A` and `B` are torch tensors of one dtype on one device -- kind as `_tensor_kind` states it --, (None, None)
    when neither is a tensor; a tensor next to anything else, two dtypes, two devices or a dtype without an entry are a ValueError"""
    torch = _torch_if_tensor(A) or _torch_if_tensor(B)
    if torch is None:
        return None, None
    _fail_if(not (isinstance(A, torch.Tensor) and isinstance(B, torch.Tensor)), "'A' and 'B' must both be torch tensors, or both NumPy arrays.")
    _fail_if(A.dtype != B.dtype, "'A' and 'B' must have the same dtype when they are torch tensors.")
    _fail_if(A.device != B.device, "'A' and 'B' must be on the same device.")
    kind = _tensor_kind(torch, A)
    _fail_if(kind is None, "'A' and 'B' must be float16, bfloat16, float32 or float64 tensors.")
    return torch, kind


def _fail_if_biases_on_half(kind, item_biases):
    _fail_if(isinstance(kind, str) and item_biases is not None,
             "'item_biases' cannot be added to 16-bit factors (a bias column in 16 bits would be rounded): pass float32 factors.")


def _fold_item_biases_tensors(torch, A, B, item_biases, n_items):
    """`_fold_item_biases` for float32 / float64 tensors: the two columns are appended on the tensors' device"""
    if isinstance(item_biases, torch.Tensor):
        item_biases = item_biases.detach().cpu().numpy()
    assert isinstance(item_biases, np.ndarray)
    _fail_if(item_biases.ndim > 2, "'item_biases' should be a 1-d array.")
    item_biases = item_biases.reshape(-1)
    _fail_if(item_biases.shape[0] == 0, "'item_biases' is empty.")
    _fail_if(item_biases.shape[0] < n_items, "Number of items in 'item_biases' must match with 'X_test'.")
    if item_biases.shape[0] > n_items:
        warn("'item_biases' has more items than 'X_test'.")
        item_biases = item_biases[:n_items]
    bias = torch.from_numpy(np.ascontiguousarray(item_biases)).to(device=B.device, dtype=B.dtype).reshape(-1, 1)
    return torch.cat([A, torch.ones((A.shape[0], 1), dtype=A.dtype, device=A.device)], dim=1), torch.cat([B, bias], dim=1)


def _half_or_typed(kind, A, B, dtype):
    """the factors of a host call, row-major with their leading dimensions: 16-bit arrays as they are, anything else in `dtype`"""
    if not isinstance(kind, str):
        A, B = A.astype(dtype, copy=False), B.astype(dtype, copy=False)
    return _row_major_with_ld(A) + _row_major_with_ld(B)


class _DeviceCall:
    """What the functions share when `scores`, or the factors `A` and `B`, are GPU tensors: the call runs on the tensor's device and
    on torch's current stream there, through the device entries; index arrays are uploaded, outputs are device tensors, and the stream
    is synchronised before they come back as NumPy arrays."""

    def __init__(self, torch, scores, kind):
        self.torch, self.kind, self.device = torch, kind, scores.device
        self.S = self.row_major(scores)
        self.out_dtype = torch.float64 if kind is np.float64 else torch.float32
        self.np_dtype = np.float64 if kind is np.float64 else np.float32
        self.keep = []                                              # the uploads live until the stream has been synchronised

    def put(self, array):
        """device address of a host array's copy (0 for None or an empty one)"""
        if array is None or array.size == 0:
            return 0
        t = self.torch.from_numpy(np.ascontiguousarray(array)).to(self.device)
        self.keep.append(t)
        return t.data_ptr()

    def empty(self, shape, dtype=None):
        return self.torch.empty(shape, dtype=dtype or self.out_dtype, device=self.device)

    @staticmethod
    def row_major(t):
        """`t` as it is when its rows are dense and ascend (a row stride is passed on), else one contiguous copy"""
        t = t.detach()
        return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()

    def run(self, entry, half_entry, **arguments):
        """`entry(dtype, S, lds, m, n, ...)` of the binding, or its 16-bit form `half_entry(kind, ...)`, on the current stream; waits"""
        self._run(entry, half_entry, (self.S.data_ptr(), self.S.stride(0), self.S.shape[0], self.S.shape[1]), arguments)

    def run_factors(self, entry, half_entry, B, **arguments):
        """the same for the factor entries, `entry(dtype, A, lda, B, ldb, m, n, k, ...)`: the call was made over `A`"""
        A, B = self.S, self.row_major(B)
        self._run(entry, half_entry, (A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), A.shape[0], B.shape[0], A.shape[1]), arguments)

    def _run(self, entry, half_entry, source, arguments):
        torch = self.torch
        with torch.cuda.device(self.device):
            _binding.load()
            _binding.set_device(self.device.index if self.device.index is not None else torch.cuda.current_device())
            stream = torch.cuda.current_stream()
            (half_entry if isinstance(self.kind, str) else entry)(self.kind, *source, stream=stream.cuda_stream, **arguments)
            stream.synchronize()
        self.keep.clear()


def calc_reco_metrics(
    X_train, X_test,
    A, B,
    k=5,
    item_biases=None,
    as_df=True,
    precision=True,
    trunc_precision=False,
    recall=False,
    average_precision=True,
    trunc_average_precision=False,
    ndcg=True,
    hit=False,
    rr=False,
    roc_auc=False,
    pr_auc=False,
    all_metrics=False,
    rename_k=True,
    break_ties_with_noise=True,
    min_pos_test=1,
    min_items_pool=2,
    consider_cold_start=True,
    cumulative=False,
    nthreads=-1,
    seed=1,
):
    """Recommendation quality metrics for implicit-feedback models, evaluated per user on an MI355X.

    Arguments, defaults and return value follow ``recometrics.calc_reco_metrics`` (reference
    recometrics/__init__.py:44-413): ``X_train`` / ``X_test`` are CSR user-item matrices with the same shape,
    ``A`` [users, factors] and ``B`` [items, factors] are the model matrices (scores are ``A @ B.T``), ``k`` the
    cut-off.  Returns a ``pandas.DataFrame`` with one row per user (``as_df=True``) or a dict of arrays plus the
    entry ``"K"``.  Users that cannot be evaluated get NaN.

    ``A`` and ``B`` may also be ``torch.Tensor``s of one dtype -- float16, bfloat16, float32 or float64 -- on one device.  16-bit
    factors are read where they lie, every factor widened exactly to float32 on the device
    (``include/recometrics_hip_half_factors.h``), and the result is float32: the same values the call returns for the tensors
    converted to float32, without the float32 copies.  CPU tensors go through the host entries without a copy; GPU tensors go through
    the device entries on their device and on torch's current stream there, which is synchronised before the result comes back in
    the usual form.  ``item_biases`` cannot be added to 16-bit factors (the bias column would be rounded).  NumPy ``float16`` arrays
    keep going through float64.

    Differences from the CPU reference, all documented in DESIGN.md: ``nthreads`` only drives the host-side sort of a matrix
    whose rows turn out unsorted (the reference sorts ``X_train`` / ``X_test`` in place; here they are never modified);
    ``break_ties_with_noise`` adds the reference's own noise (``std::mt19937(seed + user)``, reproduced bit for bit on
    the device), scores that are still exactly equal afterwards are ordered by item id; ``hit`` / ``rr`` requested
    alone are computed (the reference leaves them uninitialised) and ``pr_auc`` without ``roc_auc`` is computed from
    the full ranking.
    """
    requested = _requested_metrics(locals())
    from scipy.sparse import issparse

    if hasattr(item_biases, "to_numpy"):                 # pandas.Series
        item_biases = item_biases.to_numpy()

    # ---- factors (or the non-personalised mode: A = ones, B = biases; reference :429-436) ----
    _fail_if((A is None) != (B is None), "'A' and 'B' must either be passed together or passed as 'None' together.")
    if A is None:
        _fail_if(item_biases is None, "Must pass item biases if not passing factors.")
        A = np.ones((X_test.shape[0], 1), dtype=np.float64)
        B = np.ascontiguousarray(item_biases, dtype=np.float64).reshape(-1, 1)
        item_biases = None
    torch, kind = _factor_tensors(A, B)
    if torch is None:
        assert isinstance(A, np.ndarray) and isinstance(B, np.ndarray)
    _fail_if_biases_on_half(kind, item_biases)
    assert issparse(X_test)
    n_users, n_items = X_test.shape
    _fail_if(n_users >= _INT32_MAX, "Number of test user is larger than maximum supported.")
    _fail_if(n_items >= _INT32_MAX, "Number of items is larger than maximum supported.")
    _fail_if(X_test.data.shape[0] == 0, "'X_test' is empty.")
    A, B = _check_factors(A, B, n_users, n_items)

    # float32 only when BOTH factor matrices are float32 (reference :469); 16-bit tensors are evaluated in float32
    if torch:
        dtype = np.float64 if kind is np.float64 else np.float32
    else:
        dtype = np.float32 if (A.dtype == np.float32 and B.dtype == np.float32) else np.float64

    # ---- train matrix ----
    X_train, consider_cold_start = _train_or_empty(X_train, X_test, dtype, consider_cold_start)
    assert issparse(X_train)
    assert X_train.shape[1] == n_items
    _fail_if(X_train.shape[0] < n_users, "'X_train' and 'X_test' should have the same number of rows.")
    if X_train.shape[0] > n_users:
        warn("'X_train' mas more rows than 'X_test'.")

    _fail_if_no_ranking_metric(requested)

    # ---- scalars ----
    if isinstance(seed, np.random.RandomState):
        seed = seed.randint(_INT32_MAX)
    elif isinstance(seed, np.random.Generator):
        seed = seed.integers(_INT32_MAX)
    seed, k, nthreads = int(seed), int(k), int(nthreads)
    min_pos_test, min_items_pool = int(min_pos_test), int(min_items_pool)
    assert seed >= 1 and k >= 1 and min_pos_test >= 1 and min_items_pool >= 1
    if nthreads < 0:
        nthreads += multiprocessing.cpu_count() + 1
    assert nthreads > 0
    if nthreads > 1 and not _binding.has_openmp():
        warn("Attempting to use more than 1 thread, but package was built without multi-threading support.")
    _fail_if(k > n_items, "'k' should be smaller than the number of items.")

    if item_biases is not None:
        A, B = _fold_item_biases_tensors(torch, A, B, item_biases, n_items) if torch else _fold_item_biases(A, B, item_biases, n_items, dtype)

    # ---- normalise storage: factors in `dtype` and row-major; nothing is copied that already has the right type and layout ----
    split = _split_arrays(X_train, X_test, n_users, dtype)
    if torch and A.is_cuda:
        want = {short: requested[name] for name, short, _ in _METRICS}
        arrays = _binding._metric_outs(None, want, n_users, k, bool(cumulative), dtype)
        call = _DeviceCall(torch, A, kind)
        on_device = [call.empty(a.size) if a.size else None for a in arrays]
        train_p, train_i, test_p, test_i, test_v = split
        call.run_factors(_binding.calc_metrics_device, _binding.calc_metrics_half_device, B,
                         train_p=call.put(train_p), train_i=call.put(train_i), nnz_train=int(train_i.shape[0]),
                         test_p=call.put(test_p), test_i=call.put(test_i), test_v=call.put(test_v), nnz_test=int(test_i.shape[0]),
                         k_metrics=k, outs=[t.data_ptr() if t is not None else 0 for t in on_device], cumulative=bool(cumulative),
                         break_ties_with_noise=bool(break_ties_with_noise), consider_cold_start=bool(consider_cold_start),
                         min_items_pool=min_items_pool, min_pos_test=min_pos_test, seed=seed)
        for a, t in zip(arrays, on_device):
            if t is not None:
                a.reshape(-1)[:] = t.cpu().numpy()
        return _metrics_result(arrays, None, None, k, as_df, cumulative, rename_k)
    if torch:
        A, B = _cpu_tensor_as_array(torch, A, kind), _cpu_tensor_as_array(torch, B, kind)
    A, lda, B, ldb = _half_or_typed(kind, A, B, dtype)
    want, outs, block, keys = _output_storage(requested, n_users, dtype, as_df, cumulative)
    arrays = (_binding.calc_metrics_half if isinstance(kind, str) else _binding.calc_metrics)(
        A, lda, B, ldb, *split, k, want, bool(cumulative), bool(break_ties_with_noise),
        bool(consider_cold_start), min_items_pool, min_pos_test, nthreads, seed, outs=outs)
    return _metrics_result(arrays, block, keys, k, as_df, cumulative, rename_k)


def calc_reco_metrics_from_scores(
    X_train, X_test,
    scores,
    k=5,
    as_df=True,
    precision=True,
    trunc_precision=False,
    recall=False,
    average_precision=True,
    trunc_average_precision=False,
    ndcg=True,
    hit=False,
    rr=False,
    roc_auc=False,
    pr_auc=False,
    all_metrics=False,
    rename_k=True,
    min_pos_test=1,
    min_items_pool=2,
    consider_cold_start=True,
    cumulative=False,
    nthreads=-1,
):
    """The metrics of :func:`calc_reco_metrics` for ANY model: ``scores`` is a NumPy ``[users, items]`` array with the score of
    every item for every user -- a two-tower model with a non-linear head, an item-kNN, a re-ranker, popularity with business
    rules -- instead of the factor matrices ``A`` and ``B``.  The reference has no such call.

    ``X_train`` / ``X_test``, ``k``, the metric flags, ``all_metrics``, ``as_df``, ``rename_k``, ``min_pos_test``,
    ``min_items_pool``, ``consider_cold_start``, ``cumulative`` and ``nthreads`` mean what they mean there, with the same
    defaults, column names and return shapes; ``X_train=None`` is an empty train matrix with ``consider_cold_start=True``.
    ``scores`` must have the shape of ``X_test``; it is evaluated in float32 only when it is float32, otherwise in float64; a
    row-major array (also one with a row stride, such as a column slice of a wider matrix) is passed as it is, anything else is
    copied once.  It is never modified, and a score at a train item is never looked at.

    ``scores`` may also be a ``torch.Tensor`` of dtype float16, bfloat16, float32 or float64.  A float16 / bfloat16 tensor is read
    where it lies, every score widened exactly to float32 on the device (``include/recometrics_hip_half.h``), and the result is
    float32: the same values the call returns for the tensor converted to float32, for half the memory and half the upload.  A CPU
    tensor goes through the host entries without a copy (``stride(1) == 1`` keeps its row stride, anything else is made contiguous
    once); a GPU tensor goes through the device entries on its own device and on torch's current stream there, which is
    synchronised before the result comes back in the usual form.  A NumPy ``float16`` array keeps going through float64, as every
    NumPy dtype but float32 does: ``torch.from_numpy(x)`` selects the 16-bit path.

    There is no ``break_ties_with_noise`` and no ``seed``: the reference's tie noise exists to break the ties of a factor model
    that has not learned anything (all scores equal), and the caller of this function owns the scores -- equal scores are ordered
    by item id, the rule ``calc_reco_metrics(..., break_ties_with_noise=False)`` uses, and for scores that ARE ``A @ B.T`` as the
    library forms it the two calls return the same bits.  There is no ``item_biases`` either: add them to ``scores``.
    """
    requested = _requested_metrics(locals())
    from scipy.sparse import issparse

    torch = _torch_if_tensor(scores)
    _fail_if(torch is None and not isinstance(scores, np.ndarray), "'scores' must be a NumPy array.")
    _fail_if(scores.ndim != 2, "'scores' must be a 2-dimensional array.")
    _fail_if(not issparse(X_test), "'X_test' must be a sparse matrix.")
    n_users, n_items = X_test.shape
    _fail_if(n_users >= _INT32_MAX, "Number of test user is larger than maximum supported.")
    _fail_if(n_items >= _INT32_MAX, "Number of items is larger than maximum supported.")
    _fail_if(0 in (n_users, n_items), "Input matrices cannot be empty.")
    _fail_if(X_test.data.shape[0] == 0, "'X_test' is empty.")
    _fail_if(tuple(scores.shape) != (n_users, n_items), "'scores' and 'X_test' must have the same shape.")
    kind = _tensor_kind(torch, scores) if torch else None
    _fail_if(kind is None if torch else scores.dtype.kind not in "fiub", "'scores' must be a numeric array.")
    dtype = (np.float64 if kind is np.float64 else np.float32) if torch else np.float32 if scores.dtype == np.float32 else np.float64

    X_train, consider_cold_start = _train_or_empty(X_train, X_test, dtype, consider_cold_start)
    _fail_if(not issparse(X_train), "'X_train' must be a sparse matrix.")
    _fail_if(X_train.shape[1] != n_items, "'X_train' and 'X_test' should have the same number of columns.")
    _fail_if(X_train.shape[0] < n_users, "'X_train' and 'X_test' should have the same number of rows.")
    if X_train.shape[0] > n_users:
        warn("'X_train' mas more rows than 'X_test'.")

    _fail_if_no_ranking_metric(requested)

    k, nthreads = int(k), int(nthreads)
    min_pos_test, min_items_pool = int(min_pos_test), int(min_items_pool)
    _fail_if(k < 1, "'k' must be positive.")
    _fail_if(min_pos_test < 1 or min_items_pool < 1, "'min_pos_test' and 'min_items_pool' must be positive.")
    if nthreads < 0:
        nthreads += multiprocessing.cpu_count() + 1
    _fail_if(nthreads <= 0, "'nthreads' must be positive (or negative: counted back from the number of CPUs).")
    _fail_if(k > n_items, "'k' should be smaller than the number of items.")

    # ---- everything above raises before the library is touched ----
    split = _split_arrays(X_train, X_test, n_users, dtype)
    if torch and scores.is_cuda:
        want = {short: requested[name] for name, short, _ in _METRICS}
        arrays = _binding._metric_outs(None, want, n_users, k, bool(cumulative), dtype)
        call = _DeviceCall(torch, scores, kind)
        on_device = [call.empty(a.size) if a.size else None for a in arrays]
        train_p, train_i, test_p, test_i, test_v = split
        call.run(_binding.calc_metrics_scores_device, _binding.calc_metrics_scores_half_device,
                 train_p=call.put(train_p), train_i=call.put(train_i), nnz_train=int(train_i.shape[0]),
                 test_p=call.put(test_p), test_i=call.put(test_i), test_v=call.put(test_v), nnz_test=int(test_i.shape[0]),
                 k_metrics=k, outs=[t.data_ptr() if t is not None else 0 for t in on_device], cumulative=bool(cumulative),
                 consider_cold_start=bool(consider_cold_start), min_items_pool=min_items_pool, min_pos_test=min_pos_test)
        for a, t in zip(arrays, on_device):
            if t is not None:
                a.reshape(-1)[:] = t.cpu().numpy()
        return _metrics_result(arrays, None, None, k, as_df, cumulative, rename_k)
    want, outs, block, keys = _output_storage(requested, n_users, dtype, as_df, cumulative)
    if isinstance(kind, str):
        S, lds = _row_major_with_ld(_cpu_tensor_as_array(torch, scores, kind))
        arrays = _binding.calc_metrics_scores_half(
            S, lds, *split, k, want, bool(cumulative), bool(consider_cold_start), min_items_pool, min_pos_test, nthreads, outs=outs)
        return _metrics_result(arrays, block, keys, k, as_df, cumulative, rename_k)
    if torch:
        scores = _cpu_tensor_as_array(torch, scores, kind)
    S, lds = _row_major_with_ld(scores.astype(dtype, copy=False))
    arrays = _binding.calc_metrics_scores(
        S, lds, *split, k, want, bool(cumulative), bool(consider_cold_start), min_items_pool, min_pos_test, nthreads, outs=outs)
    return _metrics_result(arrays, block, keys, k, as_df, cumulative, rename_k)


def recommend_topk(A, B, k=10, X_train=None, item_biases=None, users=None, return_scores=True):
    """The ``k`` best items for every user, by the scores and the tie rule the metrics of :func:`calc_reco_metrics` are computed
    under (without tie noise): score descending, then item id ascending.  The reference has no such call.

    ``A`` [users, factors] and ``B`` [items, factors] as in :func:`calc_reco_metrics` (float32 only when both are float32;
    ``A=None, B=None`` with ``item_biases`` ranks by the biases alone; ``item_biases`` next to factors is added to the scores).
    ``X_train``: optional sparse user-item matrix of the items to leave out per user (any SciPy format; never modified), ``None``
    leaves nothing out.  ``users``: optional integer array -- lists for these rows of ``A`` / ``X_train`` only, in this order.
    ``A`` and ``B`` may be ``torch.Tensor``s as in :func:`calc_reco_metrics` (16-bit factors: list scores in float32; ``users`` gathers
    the rows of ``A`` where it lies).

    Returns ``(ids, scores, status)``: ``ids`` [len(users) or users, k] int32, ``scores`` of the same shape (``None`` with
    ``return_scores=False``), ``status`` int32 per row: 0 = the first ``min(k, candidates)`` places hold the list and the others
    -1 / NaN, 1 = every item is excluded, 2 = some candidate score is NaN or infinite (both: -1 / NaN everywhere).
    """
    if hasattr(item_biases, "to_numpy"):
        item_biases = item_biases.to_numpy()
    _fail_if((A is None) != (B is None), "'A' and 'B' must either be passed together or passed as 'None' together.")
    if A is None:
        _fail_if(item_biases is None, "Must pass item biases if not passing factors.")
        _fail_if(X_train is None and users is None, "Must pass 'X_train' or 'users' if not passing factors (the number of users is not known).")
        B = np.ascontiguousarray(item_biases, dtype=np.float64).reshape(-1, 1)
        n_rows = X_train.shape[0] if X_train is not None else int(np.max(np.asarray(users), initial=-1)) + 1
        A = np.ones((n_rows, 1), dtype=np.float64)
        item_biases = None
    torch, kind = _factor_tensors(A, B)
    if torch is None:
        assert isinstance(A, np.ndarray) and isinstance(B, np.ndarray)
    _fail_if_biases_on_half(kind, item_biases)
    _fail_if(A.ndim != 2, "'A' must be a 2-dimensional array.")
    _fail_if(B.ndim != 2, "'B' must be a 2-dimensional array.")
    _fail_if(A.shape[1] != B.shape[1], "'A' and 'B' must have the same number of columns.")
    _fail_if(0 in (A.shape[1], B.shape[0]), "Input matrices cannot be empty.")
    n_users, n_items = A.shape[0], B.shape[0]
    _fail_if(n_users >= _INT32_MAX, "Number of users is larger than maximum supported.")
    _fail_if(n_items >= _INT32_MAX, "Number of items is larger than maximum supported.")
    k = _list_length(k, n_items)
    if X_train is not None:
        from scipy.sparse import issparse
        _fail_if(not issparse(X_train), "'X_train' must be a sparse matrix.")
        _fail_if(X_train.shape[1] != n_items, "Number of items in 'B' and 'X_train' does not match.")
        _fail_if(X_train.shape[0] != n_users, "Number of users in 'A' and 'X_train' does not match.")
    users = _user_selection(users, n_users, "A")
    if torch:
        dtype = np.float64 if kind is np.float64 else np.float32
    else:
        dtype = np.float32 if (A.dtype == np.float32 and B.dtype == np.float32) else np.float64
    if item_biases is not None:
        A, B = _fold_item_biases_tensors(torch, A, B, item_biases, n_items) if torch else _fold_item_biases(A, B, item_biases, n_items, dtype)

    # ---- everything above raises before the library is touched ----
    if users is not None:                                    # (the one gather; a tensor's on its own device)
        A = A[torch.from_numpy(users).to(A.device)] if torch else A[users]
    excl_p, excl_i = _exclusion_csr(X_train, users)
    if A.shape[0] == 0:
        return _no_lists(k, dtype, return_scores)
    if torch and A.is_cuda:
        call = _DeviceCall(torch, A, kind)
        m = A.shape[0]
        idx, sc, st = call.empty((m, k), torch.int32), call.empty((m, k)) if return_scores else None, call.empty((m,), torch.int32)
        call.run_factors(_binding.recommend_device, _binding.recommend_half_device, B,
                         excl_p=call.put(excl_p), excl_i=call.put(excl_i), nnz_excl=0 if excl_i is None else int(excl_i.shape[0]), k_top=k,
                         idx=idx.data_ptr(), score=sc.data_ptr() if return_scores else 0, status=st.data_ptr())
        return idx.cpu().numpy(), sc.cpu().numpy() if return_scores else None, st.cpu().numpy()
    if torch:
        A, B = _cpu_tensor_as_array(torch, A, kind), _cpu_tensor_as_array(torch, B, kind)
    A, lda, B, ldb = _half_or_typed(kind, A, B, dtype)
    return (_binding.recommend_half if isinstance(kind, str) else _binding.recommend)(A, lda, B, ldb, excl_p, excl_i, k, bool(return_scores))


def recommend_topk_from_scores(scores, k=10, X_train=None, users=None, return_scores=True):
    """The ``k`` best items for every user of ANY model: :func:`recommend_topk` with the ``scores`` argument of
    :func:`calc_reco_metrics_from_scores` -- the lists those metrics are computed over.  The reference has no such call.

    ``scores``: 2-d numeric NumPy array ``[users, items]``, evaluated in float32 only when it is float32, otherwise in float64; a
    row-major array (also one with a row stride, such as a column slice of a wider matrix) is passed as it is, anything else is
    copied once.  It is never modified, and a score at an excluded item is never looked at.  Or a ``torch.Tensor`` of dtype float16,
    bfloat16, float32 or float64, on the CPU or on a GPU, as in :func:`calc_reco_metrics_from_scores`: 16-bit scores are read where
    they lie and widened exactly to float32 (list scores come back in float32), a GPU tensor is served on its device and on torch's
    current stream, ``users`` is gathered there.  A NumPy ``float16`` array keeps going through float64; ``torch.from_numpy(x)``
    selects the 16-bit path.  ``X_train``: optional sparse
    user-item matrix of the items to leave out per user (any SciPy format, int32 or int64 indices; never modified), ``None`` leaves
    nothing out.  ``users``: optional integer array -- lists for these rows of ``scores`` / ``X_train`` only, in this order (the
    rows are gathered once).  Order: score descending, then item id ascending; ``-0.0`` and ``+0.0`` are equal and come out as
    ``+0.0``.

    Returns ``(ids, scores, status)`` shaped and coded as :func:`recommend_topk` returns them.
    """
    torch = _torch_if_tensor(scores)
    _fail_if(torch is None and not isinstance(scores, np.ndarray), "'scores' must be a NumPy array.")
    _fail_if(scores.ndim != 2, "'scores' must be a 2-dimensional array.")
    kind = _tensor_kind(torch, scores) if torch else None
    _fail_if(kind is None if torch else scores.dtype.kind not in "fiub", "'scores' must be a numeric array.")
    n_users, n_items = scores.shape
    _fail_if(n_items == 0, "Input matrices cannot be empty.")
    _fail_if(n_users >= _INT32_MAX, "Number of users is larger than maximum supported.")
    _fail_if(n_items >= _INT32_MAX, "Number of items is larger than maximum supported.")
    k = _list_length(k, n_items)
    if X_train is not None:
        from scipy.sparse import issparse
        _fail_if(not issparse(X_train), "'X_train' must be a sparse matrix.")
        _fail_if(tuple(X_train.shape) != (n_users, n_items), "'scores' and 'X_train' must have the same shape.")
    users = _user_selection(users, n_users, "scores")
    dtype = (np.float64 if kind is np.float64 else np.float32) if torch else np.float32 if scores.dtype == np.float32 else np.float64

    # ---- everything above raises before the library is touched ----
    if users is not None:                                    # (the one gather: a new row-major array; a tensor's on its own device)
        scores = scores[torch.from_numpy(users).to(scores.device)] if torch else scores[users]
    excl_p, excl_i = _exclusion_csr(X_train, users)
    if scores.shape[0] == 0:
        return _no_lists(k, dtype, return_scores)
    if torch and scores.is_cuda:
        call = _DeviceCall(torch, scores, kind)
        m = scores.shape[0]
        idx, sc, st = call.empty((m, k), torch.int32), call.empty((m, k)) if return_scores else None, call.empty((m,), torch.int32)
        call.run(_binding.recommend_scores_device, _binding.recommend_scores_half_device,
                 excl_p=call.put(excl_p), excl_i=call.put(excl_i), nnz_excl=0 if excl_i is None else int(excl_i.shape[0]), k_top=k,
                 idx=idx.data_ptr(), score=sc.data_ptr() if return_scores else 0, status=st.data_ptr())
        return idx.cpu().numpy(), sc.cpu().numpy() if return_scores else None, st.cpu().numpy()
    if isinstance(kind, str):
        S, lds = _row_major_with_ld(_cpu_tensor_as_array(torch, scores, kind))
        return _binding.recommend_scores_half(S, lds, excl_p, excl_i, k, bool(return_scores))
    if torch:
        scores = _cpu_tensor_as_array(torch, scores, kind)
    S, lds = _row_major_with_ld(scores.astype(dtype, copy=False))
    return _binding.recommend_scores(S, lds, excl_p, excl_i, k, bool(return_scores))
