"""Child of tests/test_hip_factors_half.py: a fresh interpreter that imports torch BEFORE the library, then plays calc_reco_metrics and
recommend_topk with `A` / `B` as torch tensors -- float16, bfloat16, float32, float64; on the CPU, on the GPU, and on the GPU under a
stream of the caller's with the uploads of the factors still in flight on it.  Expectation: the same function on NumPy arrays with
exactly the tensors' values (16-bit tensors: widened to float32 by torch on the CPU), bit for bit.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recometrics_amd import calc_reco_metrics, recommend_topk  # noqa: E402
from recometrics_amd.synth import make_problem  # noqa: E402

M, N, KF, K, K_TOP = 70, 300, 16, 5, 7
USERS = np.array([5, 0, 33, 69])


def same_bits(a, b):
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)).all())


def main():
    from scipy.sparse import csr_array
    pr = make_problem(M, N, KF, np.float32, mean_c=20, seed=5)
    X_train = csr_array((np.ones(pr["train"][1].shape[0], np.float32), pr["train"][1], pr["train"][0]), shape=(M, N))
    X_test = csr_array((pr["test"][2], pr["test"][1], pr["test"][0]), shape=(M, N))
    failures, checked = [], 0
    side = torch.cuda.Stream()

    def metrics(A, B, noise):
        return calc_reco_metrics(X_train, X_test, A, B, k=K, all_metrics=True, as_df=False, break_ties_with_noise=noise, seed=3)

    for tdtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        A, B = torch.from_numpy(pr["A"]).to(tdtype), torch.from_numpy(pr["B"]).to(tdtype)
        half = tdtype in (torch.float16, torch.bfloat16)
        WA, WB = (A.to(torch.float32).numpy(), B.to(torch.float32).numpy()) if half else (A.numpy(), B.numpy())
        out_dtype = np.float64 if tdtype == torch.float64 else np.float32
        want_m = {noise: metrics(WA, WB, noise) for noise in (False, True)}
        want_l = recommend_topk(WA, WB, k=K_TOP, X_train=X_train, users=USERS)
        want_all = recommend_topk(WA, WB, k=K_TOP)
        for where in ("cpu", "gpu", "gpu, a stream of the caller's"):
            def tensors():
                return (A, B) if where == "cpu" else (A.cuda(non_blocking=True), B.cuda(non_blocking=True))
            ctx = torch.cuda.stream(side) if "stream" in where else torch.cuda.stream(torch.cuda.current_stream())
            with ctx:
                for noise in (False, True):
                    a, b = tensors()
                    got = metrics(a, b, noise)
                    checked += 1
                    if set(got) != set(want_m[noise]) or not all(same_bits(got[name], want_m[noise][name]) for name in got if name != "K"):
                        failures.append("%s %s metrics noise=%s" % (tdtype, where, noise))
                    if any(got[name].dtype != out_dtype for name in got if name != "K"):
                        failures.append("%s %s metrics: result dtype" % (tdtype, where))
                a, b = tensors()
                for got, want, what in ((recommend_topk(a, b, k=K_TOP, X_train=X_train, users=USERS), want_l, "users="),
                                        (recommend_topk(a, b, k=K_TOP), want_all, "everybody")):
                    checked += 1
                    if not all(same_bits(g, w) for g, w in zip(got, want)) or got[1].dtype != out_dtype:
                        failures.append("%s %s lists %s" % (tdtype, where, what))
                ids, sc, st = recommend_topk(a, b, k=K_TOP, X_train=X_train, return_scores=False)
                checked += 1
                if sc is not None or not same_bits(ids, recommend_topk(WA, WB, k=K_TOP, X_train=X_train)[0]):
                    failures.append("%s %s lists without scores" % (tdtype, where))
        if not half:                                        # item_biases next to float tensors: folded on the tensors' device
            bias = np.linspace(-1, 1, N)
            want = recommend_topk(WA, WB, k=K_TOP, item_biases=bias)
            for a, b in ((A, B), (A.cuda(), B.cuda())):
                checked += 1
                if not all(same_bits(g, w) for g, w in zip(recommend_topk(a, b, k=K_TOP, item_biases=bias), want)):
                    failures.append("%s item_biases on %s" % (tdtype, a.device))
    print(json.dumps({"ok": not failures, "checked": checked, "failures": failures}))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
