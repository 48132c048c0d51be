"""GPU: item-item models (rm_*_item_weights_*, calc_reco_metrics_from_item_weights, recommend_topk_from_item_weights): S = X_hist W
formed by k_scores_item_weights in front of the from-scores stages.

The reference of every test is the dense pair the kernel never builds: A = dense(X_hist), B = W^T.  The oracle on that pair with the
noise off (bits, ROC-AUC to one ulp: the from-scores tests' rule) and the library's own factor call on it (every bit) for the metrics;
rm_debug_scores of the pair through recommend_topk_from_scores for the lists.  History values are random and non-integer and W is
random normal, so a sum in any other order than the k-ordered chain shows in the last bit."""
import functools

import numpy as np
import pytest

from _parity import NT, hip_calc
from _util import assert_same_bits
from test_hip_entry_fields import dev  # noqa: F401 (a fixture: device copies through the HIP runtime)
from test_hip_scores import ALL, assert_all_bits, assert_like_parity, hip  # noqa: F401 (hip: a fixture)

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
M = 67
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 130)                      # the unroll of 8 and the 64-entry batch of the walk, each side of the edge
TILE = {F32: 512, F64: 256}                                     # columns of a wavefront's tile (rm_itemweights.hpp)


@functools.lru_cache(maxsize=None)
def problem(dtype, n, n_in=None, seed=0):
    """history CSR (p, i, v), W [n_in, n], train and test CSRs over n items, K, and the dense pair (A, B)"""
    n_in = n_in or n
    rng = np.random.default_rng(1000 * seed + n + n_in)
    lens = np.minimum(np.array([LENGTHS[(u + seed) % len(LENGTHS)] for u in range(M)]), n_in)
    hp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    hi = np.concatenate([np.sort(rng.choice(n_in, l, replace=False)) for l in lens]).astype(np.int32)
    hv = rng.uniform(0.5, 2.0, hi.shape[0]).astype(dtype)
    W = rng.standard_normal((n_in, n)).astype(dtype)
    ntr, nte = min(n // 4, 20), max(1, min(n // 4, 5))
    perms = [rng.permutation(n) for _ in range(M)]
    trp, tep = ((np.arange(M + 1) * c).astype(np.int32) for c in (ntr, nte))
    tri = np.concatenate([np.sort(p[:ntr]) for p in perms]).astype(np.int32)
    tei = np.concatenate([np.sort(p[ntr:ntr + nte]) for p in perms]).astype(np.int32)
    tev = rng.uniform(1.0, 2.0, tei.shape[0]).astype(dtype)
    A = np.zeros((M, n_in), dtype)
    A[np.repeat(np.arange(M), lens), hi] = hv
    for a in (hp, hi, hv, W, trp, tri, tep, tei, tev, A):
        a.setflags(write=False)
    return dict(hist=(hp, hi, hv), W=W, train=(trp, tri), test=(tep, tei, tev), K=max(1, min(5, n - 1)), A=A, B=np.ascontiguousarray(W.T))


def iw_calc(hip, pr, K, W=None, ldw=None, hist=None, cumulative=False, metrics=ALL):
    from oracle.oracle import NAMES
    W = pr["W"] if W is None else W
    want = {name: name in metrics for name in hip.METRIC_ORDER}
    outs = hip.calc_metrics_item_weights(W, ldw or W.shape[1], *(hist or pr["hist"]), *pr["train"], *pr["test"], K, want, cumulative, True, 2, 1)
    return {NAMES[name]: arr for name, arr in zip(hip.METRIC_ORDER, outs) if want[name]}


@functools.lru_cache(maxsize=None)
def reference(hip, dtype, n, n_in=None, cumulative=False):
    pr = problem(dtype, n, n_in)
    return hip_calc(hip, pr["A"], pr["B"], pr["train"], pr["test"], pr["K"], cumulative=cumulative, noise=False, dtype=dtype)


@pytest.mark.parametrize("tiles,extra", [(0, 3), (1, -1), (1, 5), (2, 1)], ids=["3", "tile-1", "tile+5", "2tile+1"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_parity_with_the_dense_pair(hip, oracle, dtype, tiles, extra):
    n = tiles * TILE[dtype] + extra
    pr = problem(dtype, n)
    for cum in (False, True):
        got = iw_calc(hip, pr, pr["K"], cumulative=cum)
        want = oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], pr["K"], cumulative=cum, noise=False, dtype=dtype, nthreads=NT)
        for name, arr in want.items():                           # (NaN == NaN must not carry the test)
            assert np.isfinite(arr).reshape(M, -1).all(axis=1).mean() >= 0.75, name
        assert_like_parity(got, want, "n=%d cumulative=%s against the oracle" % (n, cum))
        assert_all_bits(got, reference(hip, dtype, n, None, cum), "n=%d cumulative=%s against the factor call" % (n, cum))


def dev_calc(hip, dev, pr, ldw, off):
    """the device entry on the caller's layout of W: rows `ldw` elements apart, the first one `off` elements into a 256-byte-aligned
    allocation, NaN between the rows -- the stride and the base reach the kernel as they are (the host entry re-lays W)"""
    from oracle.oracle import NAMES
    dtype, (n_in, n) = pr["W"].dtype.type, pr["W"].shape
    buf = np.full(n_in * ldw + off, np.nan, dtype)
    buf[off:].reshape(n_in, ldw)[:, :n] = pr["W"]
    outs = [dev.alloc(M * dtype().nbytes) for _ in hip.METRIC_ORDER]
    hip.calc_metrics_item_weights_device(dtype, dev.put(buf) + off * dtype().nbytes, ldw, n_in, M, n, *map(dev.put, pr["hist"]), int(pr["hist"][1].shape[0]),
                                         *map(dev.put, pr["train"]), int(pr["train"][1].shape[0]), *map(dev.put, pr["test"]), int(pr["test"][1].shape[0]),
                                         pr["K"], outs)
    return {NAMES[name]: dev.get(p, (M,), dtype) for name, p in zip(hip.METRIC_ORDER, outs)}


@pytest.mark.parametrize("layout", ["stride", "base", "aligned"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_layouts_of_W(hip, dev, dtype, layout):
    """the element-load instantiation, chosen by a row stride that is no multiple of 16 bytes and by a base that is not 16-byte aligned
    under a stride that is; the vector one under a stride beyond n: the bits of the dense, aligned W"""
    ve, n = 16 // dtype().nbytes, TILE[dtype] + 5
    pr = problem(dtype, n)
    aligned = (n + 3 + ve - 1) // ve * ve
    ldw, off = {"stride": (aligned + 1, 0), "base": (aligned, 1), "aligned": (aligned, 0)}[layout]
    assert n % ve and ldw >= n + 3 and (ldw % ve != 0) == (layout == "stride")
    assert_all_bits(dev_calc(hip, dev, pr, ldw, off), reference(hip, dtype, n), "ldw = %d, base + %d" % (ldw, off))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_history_columns_that_are_not_the_items(hip, dtype):
    pr = problem(dtype, 300, 40)
    assert_all_bits(iw_calc(hip, pr, pr["K"]), reference(hip, dtype, 300, 40), "40 history columns, 300 items")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_batches_change_nothing(hip, monkeypatch, dtype):
    pr = problem(dtype, 2 * TILE[dtype] + 1)
    plain = iw_calc(hip, pr, pr["K"], cumulative=True)
    monkeypatch.setenv("RM_BATCH_USERS", "20")                   # 67 users: four batches
    assert_all_bits(iw_calc(hip, pr, pr["K"], cumulative=True), plain, "batches of 20 users")


@pytest.mark.parametrize("k", ["1", "10", "n"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lists(hip, dtype, k):
    from scipy.sparse import csr_array
    from recometrics_amd import recommend_topk_from_item_weights, recommend_topk_from_scores
    n = TILE[dtype] + 5
    pr = problem(dtype, n)
    k = n if k == "n" else int(k)
    hp, hi, hv = pr["hist"]
    X = csr_array((hv, hi, hp), shape=(M, n))
    S = hip.debug_scores(pr["A"], pr["B"]) + dtype(0)            # (-0 read as +0)
    want = recommend_topk_from_scores(S, k=k, X_train=X)
    got = recommend_topk_from_item_weights(X, pr["W"], k=k, X_train=X)
    assert (got[0] == want[0]).all() and (got[2] == want[2]).all()
    assert_same_bits(got[1], want[1], "list scores")
    empty = int(np.flatnonzero(np.diff(hp) == 0)[0])             # no history: every score +0, ids ascending
    assert (got[0][empty] == np.arange(k)).all() and not got[1][empty].view(np.uint8).any()


_DEVICE_SCRIPT = r"""
import os, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch
from scipy.sparse import csr_array
from recometrics_amd import _binding as hip, calc_reco_metrics_from_item_weights as calc, recommend_topk_from_item_weights as reco
from test_hip_item_weights import problem, iw_calc, M
from _util import assert_same_bits
from oracle.oracle import NAMES
torch.cuda.set_device(0); hip.load(); hip.set_device(0)
dev, side = torch.device("cuda", 0), torch.cuda.Stream(device=torch.device("cuda", 0))
for dtype in (np.float32, np.float64):
    n = 300
    pr = problem(dtype, n, 40)
    want = iw_calc(hip, pr, pr["K"])
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)
    W, hist, train, test = up(pr["W"]), [up(a) for a in pr["hist"]], [up(a) for a in pr["train"]], [up(a) for a in pr["test"]]
    outs = [torch.full((M,), 7.0, dtype=W.dtype, device=dev) for _ in range(10)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hip.calc_metrics_item_weights_device(dtype, W.data_ptr(), n, 40, M, n, *[t.data_ptr() for t in hist], int(hist[1].shape[0]),
                                             train[0].data_ptr(), train[1].data_ptr(), int(train[1].shape[0]),
                                             *[t.data_ptr() for t in test], int(test[1].shape[0]), pr["K"], [o.data_ptr() for o in outs],
                                             stream=side.cuda_stream)
    side.synchronize()
    for name, o in zip(hip.METRIC_ORDER, outs):
        assert_same_bits(o.cpu().numpy(), want[NAMES[name]], "device entry: " + name)
    assert hip.item_weights_kernel_ms() > 0
    # a GPU tensor through the public functions against the NumPy array through them
    X_hist, X_test = csr_array(pr["hist"][::-1], shape=(M, 40)), csr_array(pr["test"][::-1], shape=(M, n))
    X_train = csr_array((np.ones(pr["train"][1].shape[0], dtype), pr["train"][1], pr["train"][0]), shape=(M, n))
    kw = dict(k=pr["K"], X_hist=X_hist, all_metrics=True)
    assert_same_bits(calc(X_train, X_test, W, **kw).values, calc(X_train, X_test, pr["W"], **kw).values, "GPU tensor: metrics")
    view = torch.full((40, n + 3), float("nan"), dtype=W.dtype, device=dev)[:, :n]      # rows 303 elements apart: no multiple of 16 bytes
    view.copy_(W)
    assert view.stride(0) == n + 3 and (view.stride(0) * view.element_size()) %% 16
    assert_same_bits(calc(X_train, X_test, view, **kw).values, calc(X_train, X_test, pr["W"], **kw).values, "strided GPU view: metrics")
    for T in (W, view):
        got, want = reco(X_hist, T, k=7, X_train=X_train), reco(X_hist, pr["W"], k=7, X_train=X_train)
        assert (got[0] == want[0]).all() and (got[2] == want[2]).all()
        assert_same_bits(got[1], want[1], "GPU tensor: list scores")
print("ok")
"""


def test_device_entry_and_gpu_tensors():
    """device pointers on a stream that is not the default one, and a GPU tensor through the two public functions: the host entry's
    bits.  (A process of its own: the tensors are torch's, and torch wants to be loaded before the library.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT % {"root": root}], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout[-2000:] + res.stderr[-3000:]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_input_checks(hip, dtype):
    n = TILE[dtype] + 5
    pr = problem(dtype, n)
    want = reference(hip, dtype, n)
    hp, hi, hv = pr["hist"]
    rev_i, rev_v = hi.copy(), hv.copy()
    for u in range(M):                                           # every row descending, its values with it
        rev_i[hp[u]:hp[u + 1]] = hi[hp[u]:hp[u + 1]][::-1]
        rev_v[hp[u]:hp[u + 1]] = hv[hp[u]:hp[u + 1]][::-1]
    assert_all_bits(iw_calc(hip, pr, pr["K"], hist=(hp, rev_i, rev_v)), want, "unsorted history rows")
    bad = hi.copy()
    bad[hp[5]] = n
    with pytest.raises(ValueError, match=r"CSR column index out of range \[0, %d\) in row 5" % n):
        iw_calc(hip, pr, pr["K"], hist=(hp, bad, hv))
    item = int(hi[hp[3]])                                        # a non-finite row of W taints exactly the users who have that item
    W = pr["W"].copy()
    W[item] = np.nan
    has = np.array([item in hi[hp[u]:hp[u + 1]] for u in range(M)])
    got = iw_calc(hip, pr, pr["K"], W=W)
    assert has.any() and not has.all()
    for name in want:
        assert np.isnan(got[name][has]).all(), name
        assert_same_bits(got[name][~has], want[name][~has], name + " of the users without the item")
