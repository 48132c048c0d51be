#!/usr/bin/env python
"""Times the metrics from 16-bit factor matrices (rm_calc_metrics_dev_{bf16,f16}, rm_calc_metrics_bf16) against the fp32 calls at
BASELINE C2's shape: 138,493 users x 26,744 items x 64 factors, all ten metrics, k_metrics = 10, tie noise off.

    python bench_factors_half.py [--reps 5] [--warmup 1] [--out profiles/factors_half_C2.json] [--parent-f32 FILE]

C2's synthetic factors are rounded so that every value is exact in bfloat16 AND in IEEE binary16 (8 significant bits, magnitudes below
2^-14 set to zero): the three element types hold the same values, so every leg must write the same ten outputs, compared bit for bit.

Device-resident legs, device events around every call, the legs alternating within every repetition:
  f32    rm_calc_metrics_dev_f32: existing code, the yardstick;
  bf16   rm_calc_metrics_dev_bf16;
  f16    rm_calc_metrics_dev_f16;
per leg the whole call and, from rm_get_timings, the preparation and the sweep.  Condition, per 16-bit leg: its median is no larger than
the fp32 leg's median plus that leg's spread (max - min over its repetitions).
Host-entry legs, f32 against bf16, wall clock around the call: the uploads of A and B are half as large.  Reported only.  With
--c4-items the same pair at BASELINE C4's item matrix (10 M items x 128 factors, 16,384 users) when the device has the memory.
--parent-f32 FILE: a document this script wrote on the parent commit (its f32 legs are the same code): this run's f32 median must lie
within the parent's spread around the parent's median.  One JSON document."""
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
LEGS = ("f32", "bf16", "f16")
K = 10


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=0, help="fewer users than C2's (quick runs)")
    ap.add_argument("--f32-only", action="store_true", help="the f32 legs alone (a commit without the 16-bit entries)")
    ap.add_argument("--c4-items", action="store_true", help="host legs with BASELINE C4's item matrix too")
    ap.add_argument("--parent-f32", default="", help="a document of this script from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factors_half_C2.json"))
    return ap.parse_args()


def exact_in_both(X):
    """X rounded to 8 significant bits, magnitudes below 2^-14 zero: exact in bfloat16 and in IEEE binary16"""
    import torch
    W = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(torch.bfloat16).to(torch.float32)
    W[W.abs() < 2.0 ** -14] = 0
    assert bool((W.to(torch.float16).to(torch.float32) == W).all()) and bool(torch.isfinite(W).all())
    return W


def patterns(t):
    import torch
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def main():
    args = parse()
    assert args.reps >= 1
    import torch
    from recometrics_amd import _binding
    from recometrics_amd.synth import CONFIGS, make_factors, make_interactions_fast
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    legs = ("f32",) if args.f32_only else LEGS
    m, n, k, dtype, _, mean_c, seed = CONFIGS["C2"]
    if args.users:
        m = args.users
    A, B = make_factors(m, n, k, dtype, seed)
    trp, tri, tep, tei, tev = make_interactions_fast(m, n, mean_c, dtype, seed)
    WA, WB = exact_in_both(A), exact_in_both(B)
    host = {"f32": (WA.numpy(), WB.numpy()), "bf16": (patterns(WA.to(torch.bfloat16)), patterns(WB.to(torch.bfloat16)))}
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    split = [t(x) for x in (trp, tri, tep, tei, tev)]
    cast = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    F = {leg: (WA.to(cast[leg]).to(dev), WB.to(cast[leg]).to(dev)) for leg in legs}
    stream = torch.cuda.current_stream().cuda_stream
    outs = {leg: [torch.full((m,), 7.0, dtype=torch.float32, device=dev) for _ in range(10)] for leg in legs}
    torch.cuda.synchronize()

    def metrics(leg):
        a, b = F[leg]
        entry = _binding.calc_metrics_device if leg == "f32" else _binding.calc_metrics_half_device
        entry(dtype if leg == "f32" else leg, a.data_ptr(), k, b.data_ptr(), k, m, n, k, split[0].data_ptr(), split[1].data_ptr(), int(tri.shape[0]),
              split[2].data_ptr(), split[3].data_ptr(), split[4].data_ptr(), int(tei.shape[0]), K, [o.data_ptr() for o in outs[leg]], stream=stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    keys = ("prep_ms", "sweep_ms", "finalize_ms", "device_ms", "split_reused")
    call_ms, stats = {leg: [] for leg in legs}, {leg: [] for leg in legs}
    for rep in range(args.warmup + args.reps):
        for leg in legs:
            ms = timed(lambda: metrics(leg)); tm = _binding.timings()
            if rep >= args.warmup:
                call_ms[leg].append(ms); stats[leg].append({key: tm[key] for key in keys})
    torch.cuda.synchronize()
    med = statistics.median
    spread = lambda xs: max(xs) - min(xs)      # noqa: E731
    doc = {"shape": {"users": m, "items": n, "factors": k, "k_metrics": K, "nnz_train": int(tri.shape[0]), "nnz_test": int(tei.shape[0]),
                     "factor_bytes": {"f32": (m + n) * k * 4, "bf16": (m + n) * k * 2, "f16": (m + n) * k * 2}},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "device_entries": {}}
    ok = True
    for leg in legs:
        doc["device_entries"][leg] = {"call_ms": [round(x, 4) for x in call_ms[leg]], "call_median_ms": round(med(call_ms[leg]), 4),
                                      "call_spread_ms": round(spread(call_ms[leg]), 4),
                                      **{key[:-3] + "_median_ms": round(med([s[key] for s in stats[leg]]), 4) for key in keys[:4]},
                                      "split_reused": [int(s["split_reused"]) for s in stats[leg]]}
    f32 = doc["device_entries"]["f32"]
    for leg in legs[1:]:
        e = doc["device_entries"][leg]
        e["call_over_f32"] = round(e["call_median_ms"] / f32["call_median_ms"], 4)
        e["no_slower_than_f32"] = bool(e["call_median_ms"] <= f32["call_median_ms"] + f32["call_spread_ms"])
        same = all(bool(((g.view(torch.int32) == w.view(torch.int32)) | (torch.isnan(g) & torch.isnan(w))).all()) for g, w in zip(outs[leg], outs["f32"]))
        e["outputs_bit_equal"] = same
        ok = ok and same
    # ---- the host entries: the uploads of A and B are half as large ----
    want = {name: True for name in _binding.METRIC_ORDER}

    def host_pair(what, a32, b32, a16, b16, users):
        nonlocal ok
        hp = [np.ascontiguousarray(x) for x in (trp[:users + 1], tri[:trp[users]], tep[:users + 1], tei[:tep[users]], tev[:tep[users]])]
        wall, last = {"f32": [], "bf16": []}, {}
        for rep in range(args.warmup + args.reps):
            for leg in ("f32",) if args.f32_only else ("f32", "bf16"):
                a, b = (a32, b32) if leg == "f32" else (a16, b16)
                t0 = time.perf_counter()
                last[leg] = (_binding.calc_metrics if leg == "f32" else _binding.calc_metrics_half)(
                    a, a.shape[1], b, b.shape[1], *hp, K, want, False, False, True, 2, 1, 1, 1)
                if rep >= args.warmup:
                    wall[leg].append((time.perf_counter() - t0) * 1e3)
        res = {"users": users, "items": int(b32.shape[0]), "factors": int(b32.shape[1]),
               "upload_bytes": {"f32": int(a32.nbytes + b32.nbytes), "bf16": int(a32.nbytes + b32.nbytes) // 2},
               "f32": {"wall_ms": [round(x, 3) for x in wall["f32"]], "median_ms": round(med(wall["f32"]), 3)}}
        if not args.f32_only:
            same = all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(last["f32"], last["bf16"]))
            ok = ok and bool(same)
            res.update({"bf16": {"wall_ms": [round(x, 3) for x in wall["bf16"]], "median_ms": round(med(wall["bf16"]), 3)},
                        "bf16_over_f32": round(med(wall["bf16"]) / med(wall["f32"]), 4), "outputs_bit_equal": bool(same)})
        doc.setdefault("host_entries", {})[what] = res
    host_pair("C2", *host["f32"], *host["bf16"], m)
    if args.c4_items:
        m4, n4, k4 = 16384, CONFIGS["C4"][1], CONFIGS["C4"][2]
        free = torch.cuda.mem_get_info()[0]
        if free > 4 * n4 * k4 * 4:
            rng = np.random.default_rng(4)
            B4 = exact_in_both(rng.standard_normal((n4, k4), dtype=np.float32))
            A4 = exact_in_both(rng.standard_normal((m4, k4), dtype=np.float32))
            p4 = make_interactions_fast(m4, n4, CONFIGS["C4"][5], dtype, 104)
            trp, tri, tep, tei, tev = p4
            host_pair("C4_items", A4.numpy(), B4.numpy(), patterns(A4.to(torch.bfloat16)), patterns(B4.to(torch.bfloat16)), m4)
        else:
            doc["host_entries"]["C4_items"] = {"skipped": "device memory: %d bytes free" % free}
    doc["condition_holds"] = bool(all(doc["device_entries"][leg]["no_slower_than_f32"] for leg in legs[1:]))
    if args.parent_f32:
        parent = json.load(open(args.parent_f32))["device_entries"]["f32"]
        doc["parent_f32"] = {"call_median_ms": parent["call_median_ms"], "call_spread_ms": parent["call_spread_ms"], "call_ms": parent["call_ms"],
                             "f32_within_parent_spread": bool(abs(f32["call_median_ms"] - parent["call_median_ms"]) <= parent["call_spread_ms"])}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        raise SystemExit("the outputs of the legs differ")


if __name__ == "__main__":
    main()
