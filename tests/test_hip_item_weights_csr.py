"""GPU: item-item models with a sparse W (rm_*_item_weights_csr_*, k_scores_item_weights_csr).  The reference of every test is the library's
own dense entry on W.toarray(), bit for bit (tests/test_hip_item_weights.py pins that entry to the oracle); one case also asks the oracle."""
import functools

import numpy as np
import pytest

from _parity import NT
from _util import assert_same_bits
from test_hip_item_weights import M, iw_calc
from test_hip_item_weights import problem as dense_problem
from test_hip_scores import assert_all_bits, assert_like_parity, hip  # noqa: F401 (hip: a fixture)

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
TILE = {F32: 4096, F64: 2048}                                   # columns of a wavefront's tile (rm_itemweights_csr.hpp: 16 KiB of LDS)
ROW_LENGTHS = (0, 1, 63, 64, 65, 130)                           # rows of W: the 64-entry piece of the walk, each side of the edge


@functools.lru_cache(maxsize=None)
def problem(dtype, n, n_in=None):
    """tests/test_hip_item_weights.py `problem` -- history, train, test, K -- with a sparse W: its CSR (W_p, W_i, W_v), and the same dense"""
    pr = dict(dense_problem(dtype, n, n_in))
    rng = np.random.default_rng(n)
    wlens = np.minimum(np.array([ROW_LENGTHS[j % len(ROW_LENGTHS)] for j in range(n_in or n)]), n)
    wp = np.concatenate([[0], np.cumsum(wlens)]).astype(np.int32)
    wi = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in wlens]).astype(np.int32)
    rows = np.repeat(np.arange(wlens.shape[0]), wlens)
    wv = pr["W"][rows, wi]                                       # (random normal: the entries of the dense problem's W that are kept)
    W = np.zeros_like(pr["W"])
    W[rows, wi] = wv
    return dict(pr, csr=(wp, wi, wv), W=W)


def csr_calc(hip, pr, csr=None, cumulative=False):
    from oracle.oracle import NAMES
    want = dict.fromkeys(hip.METRIC_ORDER, True)
    outs = hip.calc_metrics_item_weights_csr(*(csr or pr["csr"]), pr["W"].shape[1], *pr["hist"], *pr["train"], *pr["test"], pr["K"], want, cumulative, True, 2, 1)
    return {NAMES[name]: arr for name, arr in zip(hip.METRIC_ORDER, outs)}


@functools.lru_cache(maxsize=None)
def dense(hip, dtype, n, n_in=None, cumulative=False):
    pr = problem(dtype, n, n_in)
    return iw_calc(hip, pr, pr["K"], cumulative=cumulative)


@pytest.mark.parametrize("tiles,extra", [(0, 3), (1, -1), (1, 5), (2, 1)], ids=["3", "tile-1", "tile+5", "2tile+1"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_parity_with_the_dense_entry(hip, oracle, dtype, tiles, extra):
    n = tiles * TILE[dtype] + extra
    pr = problem(dtype, n)
    wp, wi, _ = pr["csr"]
    if n > TILE[dtype]:                                         # rows of W on both sides of a tile edge
        assert any(wi[a] < TILE[dtype] <= wi[b - 1] for a, b in zip(wp[:-1], wp[1:]) if b > a)
    for cum in (False, True):
        got = csr_calc(hip, pr, cumulative=cum)
        assert_all_bits(got, dense(hip, dtype, n, None, cum), "n=%d cumulative=%s against the dense entry" % (n, cum))
        if (tiles, extra) == (1, 5):                            # ... and the oracle on the dense pair, by the from-scores rule
            want = oracle.calc(pr["A"], np.ascontiguousarray(pr["W"].T), pr["train"], pr["test"], pr["K"], cumulative=cum, noise=False, dtype=dtype, nthreads=NT)
            for name, arr in want.items():                      # (NaN == NaN must not carry the test)
                assert np.isfinite(arr).reshape(M, -1).all(axis=1).mean() >= 0.75, name
            assert_like_parity(got, want, "n=%d cumulative=%s against the oracle" % (n, cum))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_other_history_columns_and_batches(hip, monkeypatch, dtype):
    assert_all_bits(csr_calc(hip, problem(dtype, 300, 40)), dense(hip, dtype, 300, 40), "40 history columns, 300 items")
    pr = problem(dtype, 2 * TILE[dtype] + 1)
    monkeypatch.setenv("RM_BATCH_USERS", "20")                   # 67 users: four batches
    assert_all_bits(csr_calc(hip, pr, cumulative=True), dense(hip, dtype, 2 * TILE[dtype] + 1, None, True), "batches of 20 users")


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lists(hip, dtype, k):
    from scipy.sparse import csr_array
    from recometrics_amd import recommend_topk_from_item_weights as reco
    n = TILE[dtype] + 5
    hp, hi, hv = (pr := problem(dtype, n))["hist"]
    X = csr_array((hv, hi, hp), shape=(M, n))
    got, want = reco(X, csr_array(pr["csr"][::-1], shape=(n, n)), k=k, X_train=X), reco(X, pr["W"], k=k, X_train=X)
    assert (got[0] == want[0]).all() and (got[2] == want[2]).all()
    assert_same_bits(got[1], want[1], "list scores")
    empty = int(np.flatnonzero(np.diff(hp) == 0)[0])             # no history: every score +0, ids ascending
    assert (got[0][empty] == np.arange(k)).all() and not got[1][empty].view(np.uint8).any()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_rows_of_W(hip, dtype):
    n = TILE[dtype] + 5
    pr, want = problem(dtype, n), dense(hip, dtype, n)
    wp, wi, wv = pr["csr"]
    rows = np.repeat(np.arange(n), np.diff(wp))
    zr, zc = (a[::997] for a in np.nonzero(pr["W"][:128] == 0))  # explicit zeros where the first 128 rows of W store nothing
    r, c, v = np.concatenate([rows, zr]), np.concatenate([wi, zc]), np.concatenate([wv, np.zeros(zr.shape[0], dtype)])
    order = np.lexsort((c, r))
    zp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    assert_all_bits(csr_calc(hip, pr, csr=(zp, c[order].astype(np.int32), v[order])), want, "stored zeros")
    rev = wp[rows] + wp[rows + 1] - 1 - np.arange(wi.shape[0])   # every row descending, its values with it
    assert_all_bits(csr_calc(hip, pr, csr=(wp, wi[rev], wv[rev])), want, "descending rows of W")
    assert wp[6] - wp[5] == 130
    for bad_id, message in ((wi[wp[5] + 3], "CSR column index repeated in row 5"), (n, r"CSR column index out of range \[0, %d\) in row 5" % n)):
        bad = wi.copy()
        bad[wp[5] + 4] = bad_id
        with pytest.raises(ValueError, match=message):
            csr_calc(hip, pr, csr=(wp, bad, wv))
    hp, hi, _ = pr["hist"]
    j = next(int(j) for j in hi[hp[5]:hp[6]] if wp[j + 1] > wp[j])      # one stored NaN at W[j][i]: the users who have j, nobody else
    nan_v = np.where(np.arange(wv.shape[0]) == wp[j], np.nan, wv).astype(dtype)
    has = np.array([j in hi[hp[u]:hp[u + 1]] for u in range(M)])
    got = csr_calc(hip, pr, csr=(wp, wi, nan_v))
    differs = np.any([(got[name].view(np.uint8).reshape(M, -1) != want[name].view(np.uint8).reshape(M, -1)).any(axis=1) for name in want], axis=0)
    assert has.any() and not has.all() and differs[has].all() and not differs[~has].any()


_DEVICE_SCRIPT = r"""
import os, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch
from scipy.sparse import csr_array
from recometrics_amd import _binding as hip, calc_reco_metrics_from_item_weights as calc, recommend_topk_from_item_weights as reco
from test_hip_item_weights_csr import problem, csr_calc, M
from _util import assert_same_bits
from oracle.oracle import NAMES
torch.cuda.set_device(0); hip.load(); hip.set_device(0)
dev, side = torch.device("cuda", 0), torch.cuda.Stream(device=torch.device("cuda", 0))
for dtype in (np.float32, np.float64):
    n, pr = 300, problem(dtype, 300, 40)
    want = csr_calc(hip, pr)
    csr, hist, train, test = ([torch.from_numpy(np.array(a)).to(dev) for a in pr[key]] for key in ("csr", "hist", "train", "test"))
    outs = [torch.full((M,), 7.0, dtype=csr[2].dtype, device=dev) for _ in range(10)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hip.calc_metrics_item_weights_csr_device(dtype, *[t.data_ptr() for t in csr], int(csr[1].shape[0]), 40, M, n,
                                                 *[t.data_ptr() for t in hist], int(hist[1].shape[0]), *[t.data_ptr() for t in train], int(train[1].shape[0]),
                                                 *[t.data_ptr() for t in test], int(test[1].shape[0]), pr["K"], [o.data_ptr() for o in outs],
                                                 stream=side.cuda_stream)
    side.synchronize()
    for name, o in zip(hip.METRIC_ORDER, outs):
        assert_same_bits(o.cpu().numpy(), want[NAMES[name]], "device entry: " + name)
    assert hip.item_weights_kernel_ms() > 0
    X_hist, X_test = csr_array(pr["hist"][::-1], shape=(M, 40)), csr_array(pr["test"][::-1], shape=(M, n))
    X_train = csr_array((np.ones(pr["train"][1].shape[0], dtype),) + pr["train"][::-1], shape=(M, n))
    W, T = csr_array(pr["csr"][::-1], shape=(40, n)), torch.sparse_csr_tensor(csr[0].long(), csr[1].long(), csr[2], size=(40, n))
    assert_same_bits(*[calc(X_train, X_test, w, k=pr["K"], X_hist=X_hist, all_metrics=True).values for w in (T, W)], "GPU sparse tensor: metrics")
    got, want = reco(X_hist, T, k=7, X_train=X_train), reco(X_hist, W, k=7, X_train=X_train)
    assert (got[0] == want[0]).all() and (got[2] == want[2]).all()
    assert_same_bits(got[1], want[1], "GPU sparse tensor: list scores")
print("ok")
"""


def test_device_entry_and_gpu_tensors():                        # (a process of its own, as in tests/test_hip_item_weights.py)
    import os, subprocess, sys  # noqa: E401
    res = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT % {"root": os.path.dirname(os.path.dirname(os.path.abspath(__file__)))}], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout[-2000:] + res.stderr[-3000:]
