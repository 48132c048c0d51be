"""Child process of tests/test_hip_scores_half.py (torch is imported before the library, the order bench.py loads them in).
  device   the four _dev entries of include/recometrics_hip_half.h on torch device tensors and a stream that is not the default one
  python   `scores` as a CPU / GPU torch.Tensor through the two from-scores functions
Prints one JSON line: what was checked."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch                                                    # noqa: E402
from recometrics_amd import _binding as hip                     # noqa: E402
from _requests import planted_problem                           # noqa: E402
from _util import assert_same_bits                              # noqa: E402
from test_hip_recommend import check_lists                      # noqa: E402
from test_hip_recommend_scores import random_excl               # noqa: E402
from test_hip_scores import scores_calc                         # noqa: E402
from test_hip_scores_half import KINDS, NAN16, half_calc, half_lists, narrow, widen      # noqa: E402

F32 = np.float32
torch.cuda.set_device(0); hip.load(); hip.set_device(0)
dev = torch.device("cuda", 0)
TORCH16 = {"f16": torch.float16, "bf16": torch.bfloat16}


def device_entries():
    from oracle.oracle import NAMES
    side = torch.cuda.Stream(device=dev)
    m, n = 300, 5000
    ld = n + 3
    done = []
    pr = planted_problem(m, n, 16, F32, 19, 10)
    excl = random_excl(m, n, 0.01, 111, empty=(2,), full=(7,))
    xp, xi = torch.from_numpy(excl[0]).to(dev), torch.from_numpy(excl[1]).to(dev)
    trp, tri = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev) for x in pr["train"]]
    tep, tei = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev) for x in pr["test"][:2]]
    tev = torch.from_numpy(np.ascontiguousarray(pr["test"][2], F32)).to(dev)
    for kind in KINDS:
        bits = narrow(np.random.default_rng(112).standard_normal((m, n)), kind)
        wide = torch.full((m * ld + 1,), NAN16, dtype=torch.int16, device=dev)      # (+ 1: no row is 16-byte aligned but by its phase)
        view = wide[1:].view(m, ld)[:, :n]
        view.copy_(torch.from_numpy(bits.view(np.int16)).to(dev))
        W = widen(bits, kind)
        for K in (10, 1024, 1025):
            want = half_lists(hip, bits, kind, excl, K)
            check_lists(want, hip.recommend_scores(W, n, excl[0], excl[1], K), "host entry against _f32")
            idx = torch.full((m, K), 77, dtype=torch.int32, device=dev)
            sc = torch.full((m, K), 7.0, dtype=torch.float32, device=dev)
            st = torch.full((m,), 77, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            hip.recommend_scores_half_device(kind, view.data_ptr(), ld, m, n, xp.data_ptr(), xi.data_ptr(), int(xi.shape[0]), K,
                                             idx.data_ptr(), sc.data_ptr(), st.data_ptr(), side.cuda_stream)
            side.synchronize()
            check_lists((idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()), want, "%s device lists K=%d" % (kind, K))
            tm = hip.timings()
            assert tm["device_ms"] > 0 and tm["sweep_ms"] > 0 and (K > 1024 or tm["sweep_blocks"] == m), tm
            idx.fill_(77); st.fill_(77); sc.fill_(7.0)                              # score = NULL: ids only
            torch.cuda.synchronize()
            hip.recommend_scores_half_device(kind, view.data_ptr(), ld, m, n, xp.data_ptr(), xi.data_ptr(), int(xi.shape[0]), K,
                                             idx.data_ptr(), 0, st.data_ptr(), side.cuda_stream)
            side.synchronize()
            check_lists((idx.cpu().numpy(), None, st.cpu().numpy()), want, "%s device lists K=%d, ids only" % (kind, K))
            assert bool((sc == 7.0).all())
            done.append([kind, "lists %d" % K])
        K, cum = 10, True
        want = half_calc(hip, bits, kind, pr["train"], pr["test"], K, cumulative=cum)
        f32 = scores_calc(hip, W, pr["train"], pr["test"], K, cumulative=cum, dtype=F32)
        outs = [torch.full((m, K) if i < 8 else (m,), 7.0, dtype=torch.float32, device=dev) for i in range(10)]
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            hip.calc_metrics_scores_half_device(kind, view.data_ptr(), ld, m, n, trp.data_ptr(), tri.data_ptr(), int(tri.shape[0]),
                                                tep.data_ptr(), tei.data_ptr(), tev.data_ptr(), int(tei.shape[0]), K,
                                                [o.data_ptr() for o in outs], cumulative=cum, stream=side.cuda_stream)
        side.synchronize()
        for name, o in zip(hip.METRIC_ORDER, outs):
            assert_same_bits(o.cpu().numpy(), want[NAMES[name]], "%s device metrics: %s" % (kind, name))
            assert_same_bits(want[NAMES[name]], f32[NAMES[name]], "%s host metrics against _f32: %s" % (kind, name))
        done.append([kind, "metrics"])
    torch.cuda.synchronize()
    return done


def python_surface():
    from scipy.sparse import csr_array
    from recometrics_amd import calc_reco_metrics_from_scores, recommend_topk_from_scores
    m, n, K = 300, 1000, 7
    pr = planted_problem(m, n, 16, F32, 20, K)
    trp, tri = pr["train"]
    tep, tei, tev = pr["test"]
    X_train = csr_array((np.ones(tri.shape[0], F32), tri, trp), shape=(m, n))
    X_test = csr_array((tev, tei, tep), shape=(m, n))
    users = np.random.default_rng(1).permutation(m)[:97]
    base = np.random.default_rng(121).standard_normal((m, n))
    done = []
    for name in ("float16", "bfloat16", "float32", "float64"):
        tdtype = getattr(torch, name)
        wide = torch.zeros((m, n + 5), dtype=tdtype)
        wide[:, 2:2 + n] = torch.from_numpy(base).to(tdtype)
        cpu = wide[:, 2:2 + n]                                                      # a row stride: zero-copy on the CPU
        if name in ("float16", "bfloat16"):
            kind = "f16" if name == "float16" else "bf16"
            array = widen(cpu.contiguous().view(torch.int16).numpy().view(np.uint16), kind)     # W
            out_dtype = F32
        else:
            array = cpu.numpy()
            out_dtype = array.dtype
        want_lists = recommend_topk_from_scores(array, k=K, X_train=X_train)
        want_users = recommend_topk_from_scores(array, k=K, X_train=X_train, users=users)
        want_all = calc_reco_metrics_from_scores(X_train, X_test, array, k=K, all_metrics=True)
        want_dict = calc_reco_metrics_from_scores(X_train, X_test, array, k=K, as_df=False, cumulative=True)
        for where, t in (("cpu", cpu), ("cuda", cpu.to(dev))):
            if where == "cuda":
                t = torch.cat([t, t], dim=1)[:, :n]                                 # (a row stride on the device too)
                assert t.stride() == (2 * n, 1)
            got = recommend_topk_from_scores(t, k=K, X_train=X_train)
            assert got[1].dtype == out_dtype and isinstance(got[0], np.ndarray)
            check_lists(got, want_lists, "%s %s lists" % (where, name))
            check_lists(recommend_topk_from_scores(t, k=K, X_train=X_train, users=users), want_users, "%s %s users=" % (where, name))
            ids, sc, st = recommend_topk_from_scores(t, k=K, return_scores=False)
            assert sc is None and (ids == recommend_topk_from_scores(array, k=K)[0]).all()
            frame = calc_reco_metrics_from_scores(X_train, X_test, t, k=K, all_metrics=True)
            assert list(frame.columns) == list(want_all.columns) and frame.values.dtype == out_dtype
            assert_same_bits(np.ascontiguousarray(frame.values), np.ascontiguousarray(want_all.values), "%s %s frame" % (where, name))
            d = calc_reco_metrics_from_scores(X_train, X_test, t, k=K, as_df=False, cumulative=True)
            assert set(d) == set(want_dict) and d["K"] == K
            for key in want_dict:
                if key != "K":
                    assert d[key].dtype == out_dtype and d[key].shape == want_dict[key].shape
                    assert_same_bits(d[key], want_dict[key], "%s %s %s" % (where, name, key))
            done.append([where, name])
    torch.cuda.synchronize()
    return done


if __name__ == "__main__":
    print(json.dumps({"device": device_entries, "python": python_surface}[sys.argv[1]]()))
