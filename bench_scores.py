#!/usr/bin/env python
"""Times the metrics from a caller's score matrix (rm_calc_metrics_scores_dev_f32, all ten metrics) at BASELINE C2's shape.

    python bench_scores.py [--baseline-lib PATH] [--reps 5] [--warmup 1] [--out profiles/scores_C2.json]

Inputs resident in HBM; S [users x items] is made on the device from C2's synthetic factors (a matrix product; the rows of a
2,048-user stratified sample are then replaced by the library's own k-ordered fma chain, so that for those users the factor call
is a bitwise checker).  Device events around every call, the legs alternating:

  scores    rm_calc_metrics_scores_dev_f32: the whole step, and from rm_get_timings the row kernel (k_score_rows: copies and masks
            one score row per evaluated user, reduces the candidates' statistics) with its achieved bytes/s;
  copy      a plain device-to-device hipMemcpyAsync of the same users x items x 4 bytes -- the yardstick: it reads and writes what the
            row kernel reads and writes;
  baseline  `--baseline-lib`: rm_calc_metrics_dev_f32 on the same problem under RM_DEBUG_EXT_TOPK=1 in a librecometrics_hip.so built
            from the commit to compare with -- the same finalisation behind the MFMA sweep; without it "not measured".

The outputs of the LAST timed scores call are compared with the factor call of this process on the sample, bit for bit.  One JSON
document."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
METRICS = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=0, help="fewer users than C2's (quick runs)")
    ap.add_argument("--sample", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores_C2.json"))
    return ap.parse_args()


def stratified_sample(test_p, m, count, seed=0):
    """the first and the last users, the shortest and the longest test rows (the longest are the users with the deepest tables of
    positives), the rest at random"""
    order = np.argsort(np.diff(test_p), kind="stable")
    edge = min(128, max(1, count // 16))
    pick = set(range(edge)) | set(range(m - edge, m)) | set(order[:edge].tolist()) | set(order[-edge:].tolist())
    for u in np.random.default_rng(seed).permutation(m):
        if len(pick) >= min(count, m):
            break
        pick.add(int(u))
    return np.array(sorted(pick), np.int64)


def baseline_entry(path):
    """rm_calc_metrics_dev_f32 of another build of the library, loaded with RM_DEBUG_EXT_TOPK=1 in the environment (the library reads
    its switches once, when it is loaded: this process's own copy, loaded before, does not see it)"""
    os.environ["RM_DEBUG_EXT_TOPK"] = "1"
    try:
        lib = C.CDLL(path)
    finally:
        del os.environ["RM_DEBUG_EXT_TOPK"]
    vp, i32, i64, u64, sz, ci = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_int
    fn = lib.rm_calc_metrics_dev_f32
    fn.argtypes = [vp, sz, vp, sz, i32, i32, i32, vp, vp, i64, vp, vp, vp, i64, i32, ci, ci] + [vp] * 10 + [ci, i32, i32, u64, vp]
    fn.restype = ci
    lib.rm_last_error.restype = C.c_char_p
    lib.rm_get_timings.argtypes = [C.POINTER(C.c_double), ci]
    return lib, fn


def main():
    args = parse()
    import torch
    from recometrics_amd import _binding
    from recometrics_amd.synth import CONFIGS, make_factors, make_interactions_fast
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    m, n, k, dtype, K, mean_c, seed = CONFIGS["C2"]
    if args.users:
        m = args.users
    A, B = make_factors(m, n, k, dtype, seed)
    trp, tri, tep, tei, tev = make_interactions_fast(m, n, mean_c, dtype, seed)
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    dA, dB, dtrp, dtri, dtep, dtei, dtev = t(A), t(B), t(trp), t(tri), t(tep), t(tei), t(tev)
    stream = torch.cuda.current_stream().cuda_stream
    # S on the device; the sample's rows by the library's own chain (rm_debug_scores: the sweep's contraction, bit-identical to it)
    dS = dA @ dB.T
    users = stratified_sample(tep, m, args.sample)
    dS[torch.from_numpy(users).to(dev)] = t(_binding.debug_scores(A[users], B))
    copy_dst = torch.empty_like(dS)
    torch.cuda.synchronize()
    hiprt = C.CDLL("libamdhip64.so")
    hiprt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hiprt.hipMemcpyAsync.restype = C.c_int
    base = baseline_entry(args.baseline_lib) if args.baseline_lib else None
    outs = [torch.empty(m, dtype=torch.float32, device=dev) for _ in METRICS]
    outs_f = [torch.empty(m, dtype=torch.float32, device=dev) for _ in METRICS]
    vp = lambda x: C.c_void_p(int(x)) if x else None                    # noqa: E731

    def scores():
        _binding.calc_metrics_scores_device(dtype, dS.data_ptr(), n, m, n, dtrp.data_ptr(), dtri.data_ptr(), int(tri.shape[0]),
                                            dtep.data_ptr(), dtei.data_ptr(), dtev.data_ptr(), int(tei.shape[0]), K,
                                            [o.data_ptr() for o in outs], stream=stream)

    def copy():
        rc = hiprt.hipMemcpyAsync(vp(copy_dst.data_ptr()), vp(dS.data_ptr()), m * n * 4, 3, vp(stream))      # 3 = device to device
        if rc:
            raise RuntimeError("hipMemcpyAsync failed (%d)" % rc)

    def factor(fn=None, into=outs_f):
        if fn is None:
            _binding.calc_metrics_device(dtype, dA.data_ptr(), k, dB.data_ptr(), k, m, n, k, dtrp.data_ptr(), dtri.data_ptr(), int(tri.shape[0]),
                                         dtep.data_ptr(), dtei.data_ptr(), dtev.data_ptr(), int(tei.shape[0]), K, [o.data_ptr() for o in into],
                                         break_ties_with_noise=False, stream=stream)
            return
        rc = fn(vp(dA.data_ptr()), k, vp(dB.data_ptr()), k, m, n, k, vp(dtrp.data_ptr()), vp(dtri.data_ptr()), int(tri.shape[0]),
                vp(dtep.data_ptr()), vp(dtei.data_ptr()), vp(dtev.data_ptr()), int(tei.shape[0]), K, 0, 0,
                *[vp(o.data_ptr()) for o in into], 1, 2, 1, 1, vp(stream))
        if rc:
            raise RuntimeError("baseline call failed (%d): %s" % (rc, base[0].rm_last_error().decode(errors="replace")))

    outs_b = [torch.empty(m, dtype=torch.float32, device=dev) for _ in METRICS] if base else None
    baseline = (lambda: factor(base[1], outs_b)) if base else None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        scores(); copy()
        if base:
            baseline()
    torch.cuda.synchronize()
    t_scores, t_copy, t_base, splits, base_splits = [], [], [], [], []
    for _ in range(args.reps):
        t_scores.append(timed(scores))
        tm = _binding.timings()
        splits.append({key: tm[key] for key in ("prep_ms", "sweep_ms", "finalize_ms", "device_ms", "sweep_blocks")})
        t_copy.append(timed(copy))
        if base:
            t_base.append(timed(baseline))
            buf = (C.c_double * 10)()
            base[0].rm_get_timings(buf, 10)
            base_splits.append({"prep_ms": buf[0], "sweep_ms": buf[1], "finalize_ms": buf[2], "device_ms": buf[3]})
    torch.cuda.synchronize()
    # the outputs of the last timed call against the factor call of this process, on the sample, bit for bit
    factor()
    torch.cuda.synchronize()
    du = torch.from_numpy(users).to(dev)
    differing = {}
    for name, a, b in zip(METRICS, outs, outs_f):
        x, y = a[du].cpu().numpy(), b[du].cpu().numpy()
        same = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        differing[name] = int((~same).sum())
    evaluated = int((~torch.isnan(outs[0])).sum().item())
    parity = {"users_checked": int(users.shape[0]), "users_evaluated_in_the_sample": int((~torch.isnan(outs[0][du])).sum().item()),
              "differing_values_per_metric": differing, "bit_equal": not any(differing.values())}
    med = lambda xs: statistics.median(xs)                               # noqa: E731
    rows = int(splits[-1]["sweep_blocks"])
    row_ms = med([s["sweep_ms"] for s in splits])
    row_ld = (n + 63) // 64 * 64
    row_bytes = rows * (n + row_ld) * 4
    copy_ms = med(t_copy)
    doc = {"shape": {"users": m, "items": n, "dtype": np.dtype(dtype).name, "k_metrics": K, "metrics": "all ten",
                     "nnz_train": int(tri.shape[0]), "nnz_test": int(tei.shape[0]), "score_matrix_bytes": m * n * 4},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "scores_step_ms": [round(x, 4) for x in t_scores], "scores_step_median_ms": round(med(t_scores), 4),
           "scores_users_per_s": round(m / med(t_scores) * 1e3), "users_evaluated": evaluated,
           "scores_timings_median_ms": {key: round(med([s[key] for s in splits]), 4) for key in ("prep_ms", "sweep_ms", "finalize_ms", "device_ms")},
           "row_kernel": {"rows": rows, "median_ms": round(row_ms, 4), "bytes_read_and_written": row_bytes,
                          "achieved_bytes_per_s": round(row_bytes / (row_ms * 1e-3)) if row_ms > 0 else None},
           "copy_yardstick": {"what": "hipMemcpyAsync device to device, users x items x 4 bytes", "bytes_read_and_written": 2 * m * n * 4,
                              "ms": [round(x, 4) for x in t_copy], "median_ms": round(copy_ms, 4),
                              "achieved_bytes_per_s": round(2 * m * n * 4 / (copy_ms * 1e-3))},
           "row_kernel_over_copy": round(row_ms / copy_ms, 4), "row_kernel_per_byte_over_copy_per_byte": round((row_ms / row_bytes) / (copy_ms / (2 * m * n * 4)), 4),
           "target_row_kernel_at_most_1_5x_copy": bool(row_ms <= 1.5 * copy_ms),
           "parity_vs_factor_call": parity}
    if base:
        same_b = all(bool(((a[du] == b[du]) | (torch.isnan(a[du]) & torch.isnan(b[du]))).all().item()) for a, b in zip(outs, outs_b))
        doc["baseline"] = {"what": "rm_calc_metrics_dev_f32 under RM_DEBUG_EXT_TOPK=1, library built from the parent commit",
                           "ms": [round(x, 4) for x in t_base], "median_ms": round(med(t_base), 4),
                           "timings_median_ms": {key: round(med([s[key] for s in base_splits]), 4) for key in base_splits[0]},
                           "scores_step_over_baseline": round(med(t_scores) / med(t_base), 4), "outputs_equal_on_the_sample": same_b}
    else:
        doc["baseline"] = "not measured"
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not parity["bit_equal"]:
        raise SystemExit("the timed outputs differ from the factor call's on the sample")


if __name__ == "__main__":
    main()
