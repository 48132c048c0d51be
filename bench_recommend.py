#!/usr/bin/env python
"""Times the recommendation lists (rm_recommend_dev_f32, every user) at BASELINE C2's shape against the nearest thing the library
could do before they existed: rm_calc_metrics_dev_f32 asking for precision alone (the same sweep family; it skips the users it
cannot evaluate and hands no list back).

    python bench_recommend.py [--baseline-lib PATH] [--reps 7] [--warmup 2] [--K 10 100] [--out profiles/recommend_C2.json]

Inputs resident in HBM, device events around every call, the two calls alternating.  `--baseline-lib`: a librecometrics_hip.so built
from the commit to compare with; without it the baseline is written as "not measured".  The lists of the LAST timed call are checked
against the oracle restatement on a stratified sample of 2,048 users (scores by the k-ordered fma chain, order by (score descending,
item ascending)).  One JSON document."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--K", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--users", type=int, default=0, help="fewer users than C2's (quick runs)")
    ap.add_argument("--sample", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_C2.json"))
    return ap.parse_args()


def expected_lists(S, excl, K, users):
    p, i = excl
    n = S.shape[1]
    ids = np.full((users.shape[0], K), -1, np.int32)
    sc = np.full((users.shape[0], K), np.nan, S.dtype)
    st = np.zeros(users.shape[0], np.int32)
    for r, u in enumerate(users):
        keep = np.ones(n, bool)
        keep[i[p[u]:p[u + 1]]] = False
        cand = np.flatnonzero(keep)
        if cand.shape[0] == 0:
            st[r] = 1
            continue
        s = S[r, cand]
        if not np.isfinite(s).all():
            st[r] = 2
            continue
        o = np.lexsort((cand, -s))[:K]
        ids[r, :o.shape[0]] = cand[o]
        sc[r, :o.shape[0]] = s[o]
    return ids, sc, st


def stratified_sample(excl_p, m, count, seed=0):
    order = np.argsort(np.diff(excl_p), kind="stable")
    edge = min(128, max(1, count // 16))
    pick = set(range(edge)) | set(range(m - edge, m)) | set(order[:edge].tolist()) | set(order[-edge:].tolist())
    for u in np.random.default_rng(seed).permutation(m):
        if len(pick) >= min(count, m):
            break
        pick.add(int(u))
    return np.array(sorted(pick), np.int64)


def baseline_entry(path):
    """rm_calc_metrics_dev_f32 of another build of the library (its own copy of every global)"""
    lib = C.CDLL(path)
    vp, i32, i64, u64, sz, ci = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_int
    fn = lib.rm_calc_metrics_dev_f32
    fn.argtypes = [vp, sz, vp, sz, i32, i32, i32, vp, vp, i64, vp, vp, vp, i64, i32, ci, ci] + [vp] * 10 + [ci, i32, i32, u64, vp]
    fn.restype = ci
    lib.rm_last_error.restype = C.c_char_p
    return lib, fn


def main():
    args = parse()
    import torch
    from oracle.oracle import Oracle
    from recometrics_amd import _binding
    from recometrics_amd.synth import CONFIGS, make_factors, make_interactions_fast
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    m, n, k, dtype, _, mean_c, seed = CONFIGS["C2"]
    if args.users:
        m = args.users
    A, B = make_factors(m, n, k, dtype, seed)
    trp, tri, tep, tei, tev = make_interactions_fast(m, n, mean_c, dtype, seed)
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    dA, dB, dtrp, dtri, dtep, dtei, dtev = t(A), t(B), t(trp), t(tri), t(tep), t(tei), t(tev)
    stream = torch.cuda.current_stream().cuda_stream
    base = baseline_entry(args.baseline_lib) if args.baseline_lib else None
    users = stratified_sample(trp, m, args.sample)
    S = Oracle().scores(A[users], B, dtype=dtype)
    doc = {"shape": {"users": m, "items": n, "factors": k, "dtype": np.dtype(dtype).name, "nnz_excluded": int(tri.shape[0])},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "baseline": "rm_calc_metrics_dev_f32, precision only, from a library built from the parent commit" if args.baseline_lib else "not measured",
           "cases": []}
    ok = True
    for K in args.K:
        idx = torch.empty((m, K), dtype=torch.int32, device=dev)
        sc = torch.empty((m, K), dtype=torch.float32, device=dev)
        st = torch.empty(m, dtype=torch.int32, device=dev)
        p_at_k = torch.empty(m, dtype=torch.float32, device=dev)

        def reco():
            _binding.recommend_device(dtype, dA.data_ptr(), k, dB.data_ptr(), k, m, n, k, dtrp.data_ptr(), dtri.data_ptr(), int(tri.shape[0]), K,
                                      idx.data_ptr(), sc.data_ptr(), st.data_ptr(), stream)

        def metric():
            vp = lambda x: C.c_void_p(int(x)) if x else None                # noqa: E731
            rc = base[1](vp(dA.data_ptr()), k, vp(dB.data_ptr()), k, m, n, k, vp(dtrp.data_ptr()), vp(dtri.data_ptr()), int(tri.shape[0]),
                         vp(dtep.data_ptr()), vp(dtei.data_ptr()), vp(dtev.data_ptr()), int(tei.shape[0]), K, 0, 0,
                         vp(p_at_k.data_ptr()), *([None] * 9), 1, 2, 1, 1, vp(stream))
            if rc:
                raise RuntimeError("baseline call failed (%d): %s" % (rc, base[0].rm_last_error().decode(errors="replace")))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(args.warmup):
            reco()
            if base:
                metric()
        torch.cuda.synchronize()
        t_reco, t_base, splits = [], [], []
        for _ in range(args.reps):
            t_reco.append(timed(reco))
            tm = _binding.timings()
            splits.append({key: tm[key] for key in ("prep_ms", "sweep_ms", "finalize_ms", "device_ms")})
            if base:
                t_base.append(timed(metric))
        torch.cuda.synchronize()
        # the lists of the last timed call
        t0 = time.time()
        hi, hs, hst = idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()
        wi, ws, wst = expected_lists(S, (trp, tri), K, users)
        same_scores = (hs[users].view(np.uint32) == ws.view(np.uint32)) | (np.isnan(hs[users]) & np.isnan(ws))
        parity = {"users_checked": int(users.shape[0]), "status_equal": bool((hst[users] == wst).all()),
                  "ids_equal": bool((hi[users] == wi).all()), "scores_bit_equal": bool(same_scores.all()),
                  "status_counts": {str(v): int((hst == v).sum()) for v in (0, 1, 2)}, "seconds": round(time.time() - t0, 1)}
        ok = ok and parity["status_equal"] and parity["ids_equal"] and parity["scores_bit_equal"]
        med = statistics.median(t_reco)
        case = {"K": K, "recommend_ms": [round(x, 4) for x in t_reco], "recommend_median_ms": round(med, 4),
                "recommend_users_per_s": round(m / med * 1e3),
                "recommend_timings_median_ms": {key: round(statistics.median(s[key] for s in splits), 4) for key in splits[0]},
                "parity": parity}
        if base:
            bmed = statistics.median(t_base)
            case.update({"baseline_ms": [round(x, 4) for x in t_base], "baseline_median_ms": round(bmed, 4),
                         "baseline_min_max_ms": [round(min(t_base), 4), round(max(t_base), 4)],
                         "baseline_users_evaluated": int((~torch.isnan(p_at_k)).sum().item()),
                         "recommend_over_baseline": round(med / bmed, 4),
                         "recommend_median_minus_baseline_median_ms": round(med - bmed, 4),
                         "recommend_no_slower_than_baseline_median_plus_its_spread": bool(med <= bmed + max(t_base) - min(t_base))})
        else:
            case.update({"baseline_ms": "not measured", "baseline_median_ms": "not measured"})
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        raise SystemExit("the timed lists differ from the oracle's")


if __name__ == "__main__":
    main()
