#!/usr/bin/env python
"""Times the top-K lists from a 16-bit score matrix (rm_recommend_scores_dev_{bf16,f16}) against the fp32 call at BASELINE C2's shape.

    python bench_scores_half.py [--reps 5] [--warmup 1] [--out profiles/scores_half_C2.json]

Scores resident in HBM.  W [users x items] fp32 is made on the device from C2's synthetic factors and rounded so that every value is
exact in bfloat16 AND in IEEE binary16 (8 significant bits, magnitudes below 2^-14 set to zero); S_bf16 and S_f16 hold the same values
in 16 bits, so the three legs must write the same lists.  Device events around every call, the legs alternating within every
repetition, at k_top = 10 and 100:

  f32    rm_recommend_scores_dev_f32 on W: existing code, the yardstick;
  bf16   rm_recommend_scores_dev_bf16 on S_bf16;
  f16    rm_recommend_scores_dev_f16 on S_f16;

per leg the whole call and, from rm_get_timings, the row kernel (k_topk_rows) with its achieved bytes/s.  The lists of the last call of
every leg are compared bit for bit.  One more pair of legs goes through the HOST entries at 16,384 users (f32 against bf16, wall clock
around the call): the upload of the scores is half as large there.

Condition, per k_top and per 16-bit leg: its median is no larger than the fp32 leg's median plus that leg's spread (max - min over
its repetitions).  One JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
K_TOPS = (10, 100)
LEGS = ("f32", "bf16", "f16")
HOST_USERS = 16384


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=0, help="fewer users than C2's (quick runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores_half_C2.json"))
    return ap.parse_args()


def main():
    args = parse()
    assert args.reps >= 1
    import torch
    from recometrics_amd import _binding
    from recometrics_amd.synth import CONFIGS, make_factors, make_interactions_fast
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    m, n, k, dtype, _, mean_c, seed = CONFIGS["C2"]
    if args.users:
        m = args.users
    A, B = make_factors(m, n, k, dtype, seed)
    trp, tri = make_interactions_fast(m, n, mean_c, dtype, seed)[:2]
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    dtrp, dtri = t(trp), t(tri)
    stream = torch.cuda.current_stream().cuda_stream
    # W: exact in both 16-bit formats
    W = (t(A) @ t(B).T).to(torch.bfloat16).to(torch.float32)
    W[W.abs() < 2.0 ** -14] = 0
    S = {"f32": W, "bf16": W.to(torch.bfloat16), "f16": W.to(torch.float16)}
    assert bool((S["bf16"].to(torch.float32) == W).all()) and bool((S["f16"].to(torch.float32) == W).all()) and bool(torch.isfinite(W).all())
    torch.cuda.synchronize()
    outs = {(leg, K): (torch.empty((m, K), dtype=torch.int32, device=dev), torch.empty((m, K), dtype=torch.float32, device=dev),
                       torch.empty(m, dtype=torch.int32, device=dev)) for leg in LEGS for K in K_TOPS}

    def lists(leg, K):
        idx, sc, st = outs[leg, K]
        tail = (dtrp.data_ptr(), dtri.data_ptr(), int(tri.shape[0]), K, idx.data_ptr(), sc.data_ptr(), st.data_ptr(), stream)
        if leg == "f32":
            _binding.recommend_scores_device(dtype, W.data_ptr(), n, m, n, *tail)
        else:
            _binding.recommend_scores_half_device(leg, S[leg].data_ptr(), n, m, n, *tail)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    keys = ("prep_ms", "sweep_ms", "finalize_ms", "device_ms", "sweep_blocks")
    call_ms = {key: [] for key in outs}
    stats = {key: [] for key in outs}
    for rep in range(args.warmup + args.reps):
        for K in K_TOPS:
            for leg in LEGS:
                ms = timed(lambda: lists(leg, K)); tm = _binding.timings()
                if rep >= args.warmup:
                    call_ms[leg, K].append(ms); stats[leg, K].append({key: tm[key] for key in keys})
    torch.cuda.synchronize()
    med = statistics.median
    doc = {"shape": {"users": m, "items": n, "k_top": list(K_TOPS), "nnz_excl": int(tri.shape[0]),
                     "score_matrix_bytes": {"f32": m * n * 4, "bf16": m * n * 2, "f16": m * n * 2}},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "device_entries": {}, "lists_bit_equal": {}}
    ok = True
    for K in K_TOPS:
        legs = {}
        for leg in LEGS:
            kern = [s["sweep_ms"] for s in stats[leg, K]]
            nbytes = m * n * (4 if leg == "f32" else 2)
            legs[leg] = {"call_ms": [round(x, 4) for x in call_ms[leg, K]], "call_median_ms": round(med(call_ms[leg, K]), 4),
                         "row_kernel_ms": [round(x, 4) for x in kern], "row_kernel_median_ms": round(med(kern), 4),
                         "row_kernel_spread_ms": round(max(kern) - min(kern), 4), "row_kernel_blocks": int(stats[leg, K][-1]["sweep_blocks"]),
                         "row_kernel_bytes_read": nbytes, "row_kernel_achieved_bytes_per_s": round(nbytes / (med(kern) * 1e-3)) if med(kern) > 0 else None}
        f32 = legs["f32"]
        for leg in LEGS[1:]:
            legs[leg]["row_kernel_over_f32"] = round(legs[leg]["row_kernel_median_ms"] / f32["row_kernel_median_ms"], 4) if f32["row_kernel_median_ms"] > 0 else None
            legs[leg]["no_slower_than_f32"] = bool(legs[leg]["row_kernel_median_ms"] <= f32["row_kernel_median_ms"] + f32["row_kernel_spread_ms"])
            legs[leg]["call_no_slower_than_f32"] = bool(legs[leg]["call_median_ms"] <= f32["call_median_ms"] + max(call_ms["f32", K]) - min(call_ms["f32", K]))
        doc["device_entries"][str(K)] = legs
        same = {}
        for leg in LEGS[1:]:
            (gi, gs, gt), (fi, fs, ft) = outs[leg, K], outs["f32", K]
            same_s = (gs.view(torch.int32) == fs.view(torch.int32)) | (torch.isnan(gs) & torch.isnan(fs))
            same[leg] = bool((gi == fi).all()) and bool(same_s.all()) and bool((gt == ft).all())
            ok = ok and same[leg]
        doc["lists_bit_equal"][str(K)] = same
    # ---- the host entries at 16,384 users: the upload is half as large ----
    mh, K = min(HOST_USERS, m), K_TOPS[0]
    hW = W[:mh].cpu().numpy()
    hS = S["bf16"][:mh].cpu().view(torch.int16).numpy().view(np.uint16)
    hp, hi = np.ascontiguousarray(trp[:mh + 1]), np.ascontiguousarray(tri[:trp[mh]])
    wall = {"f32": [], "bf16": []}
    last = {}
    for rep in range(args.warmup + args.reps):
        for leg in ("f32", "bf16"):
            t0 = time.perf_counter()
            last[leg] = _binding.recommend_scores(hW, n, hp, hi, K) if leg == "f32" else _binding.recommend_scores_half(hS, n, hp, hi, K)
            if rep >= args.warmup:
                wall[leg].append((time.perf_counter() - t0) * 1e3)
    host_same = bool((last["f32"][0] == last["bf16"][0]).all() and (last["f32"][1].view(np.uint32) == last["bf16"][1].view(np.uint32)).all()
                     and (last["f32"][2] == last["bf16"][2]).all())
    ok = ok and host_same
    doc["host_entries"] = {"users": mh, "k_top": K, "upload_bytes": {"f32": mh * n * 4, "bf16": mh * n * 2},
                           "f32": {"wall_ms": [round(x, 3) for x in wall["f32"]], "median_ms": round(med(wall["f32"]), 3)},
                           "bf16": {"wall_ms": [round(x, 3) for x in wall["bf16"]], "median_ms": round(med(wall["bf16"]), 3)},
                           "bf16_over_f32": round(med(wall["bf16"]) / med(wall["f32"]), 4),
                           "no_slower_than_f32": bool(med(wall["bf16"]) <= med(wall["f32"]) + max(wall["f32"]) - min(wall["f32"])),
                           "lists_bit_equal": host_same}
    doc["condition_holds"] = bool(all(doc["device_entries"][str(K)][leg]["no_slower_than_f32"] for K in K_TOPS for leg in LEGS[1:]))
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        raise SystemExit("the lists of the three legs differ")


if __name__ == "__main__":
    main()
