#!/usr/bin/env python
"""Times the metrics over per-user candidate sets (rm_calc_metrics_candidates_dev_f32, k_metrics_candidates).

    python bench_metrics_candidates.py [--reps 5] [--warmup 1] [--out profiles/metrics_candidates.json]

fp32, inputs resident in HBM, device events around every call, medians, the legs alternating within every repetition.  Item matrices:
BASELINE C2's (26,744 x 64) and the north star's (1,000,000 x 128); 16,384 users; 100 and 1,024 distinct candidates per user (one from
every stratum of the catalogue), 1 and 10 test items per user among them; K = 10, all ten metrics.  Per leg: ms per call and for the two
launches of the kernel alone (rm_get_timings), kernel time per user, and next to it

  floor        rm_recommend_candidates_dev_f32 on the same rows at k_top = K: the gather, the scores and a selection, no metric;
  comparison   the only device route there was: rm_calc_metrics_dev_f32 with the COMPLEMENT of the candidate rows as the train matrix,
               at the north star's item matrix, for the first --complement-users users (m (n - C) train entries have to fit), with the
               new call timed on the same users right in front of it; its ten outputs are compared bit for bit with the new call's.
               Condition: the new call's median plus its own spread (max - min) lies below the complement call's median.

One JSON document."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
K = 10
CATALOGUES = (("C2", 26_744, 64), ("NS", 1_000_000, 128))
CANDIDATES, TEST_ITEMS = (100, 1024), (1, 10)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=16384)
    ap.add_argument("--complement-users", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_candidates.json"))
    return ap.parse_args()


def main():
    args = parse()
    import torch
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    assert args.reps >= 5, "medians of at least five calls"
    dev, m, mc, dtype = torch.device("cuda:0"), args.users, args.complement_users, np.float32
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def metric_outputs(users):
        return [torch.empty(users, dtype=torch.float32, device=dev) for _ in range(10)]

    legs, items = {}, {}
    for name, n, k in CATALOGUES:
        items[name] = (torch.randn((m, k), generator=gen, device=dev) / k ** 0.5, torch.randn((n, k), generator=gen, device=dev) / k ** 0.5, n, k)
        for c in CANDIDATES:
            stride = n // c                                          # candidate j of a user: one id of stratum j -- distinct and sorted
            rows = (torch.arange(c, device=dev) * stride).unsqueeze(0) + torch.randint(stride, (m, c), generator=gen, device=dev)
            cp = (torch.arange(m + 1, device=dev) * c).to(torch.int32)
            for t in TEST_ITEMS:
                at = torch.linspace(0, c - 1, t, device=dev).round().long()
                legs[(name, c, t)] = {"cp": cp, "ci": rows.to(torch.int32).reshape(-1).contiguous(), "tp": (torch.arange(m + 1, device=dev) * t).to(torch.int32),
                                      "ti": rows[:, at].to(torch.int32).reshape(-1).contiguous(), "tv": torch.ones(m * t, dtype=torch.float32, device=dev),
                                      "out": metric_outputs(m), "lists": (torch.empty((m, K), dtype=torch.int32, device=dev), torch.empty((m, K), dtype=torch.float32, device=dev),
                                                                          torch.empty(m, dtype=torch.int32, device=dev)),
                                      "c": c, "t": t, "call_ms": [], "kernel_ms": [], "floor_ms": [], "floor_kernel_ms": [], "blocks": 0}

    def metrics(name, leg, users, out):
        A, B, n, k = items[name]
        _binding.calc_metrics_candidates_device(dtype, A.data_ptr(), k, B.data_ptr(), k, users, n, k, leg["cp"].data_ptr(), leg["ci"].data_ptr(), users * leg["c"],
                                                leg["tp"].data_ptr(), leg["ti"].data_ptr(), leg["tv"].data_ptr(), users * leg["t"], K,
                                                [o.data_ptr() for o in out], stream=stream)

    def lists(name, leg):
        A, B, n, k = items[name]
        _binding.recommend_candidates_device(dtype, A.data_ptr(), k, B.data_ptr(), k, m, n, k, leg["cp"].data_ptr(), leg["ci"].data_ptr(), m * leg["c"], K,
                                             *(x.data_ptr() for x in leg["lists"]), stream)

    # the comparison's train matrices: the complement of the first `mc` candidate rows of the north star's legs
    comps, n = {}, items["NS"][2]
    for c in CANDIDATES:
        listed = torch.zeros((mc, n), dtype=torch.bool, device=dev)
        listed.scatter_(1, legs[("NS", c, TEST_ITEMS[0])]["ci"][:mc * c].reshape(mc, c).long(), True)
        rest = torch.nonzero(~listed)[:, 1].to(torch.int32).contiguous()      # (sorted by user, then by item)
        for t in TEST_ITEMS:
            comps[(c, t)] = {"p": (torch.arange(mc + 1, device=dev) * (n - c)).to(torch.int32), "i": rest, "nnz": int(rest.shape[0]),
                             "out": metric_outputs(mc), "new_out": metric_outputs(mc), "ms": [], "new_ms": []}
        del listed
    torch.cuda.synchronize()

    def complement(c, t):
        A, B, n, k = items["NS"]
        leg, cm = legs[("NS", c, t)], comps[(c, t)]
        _binding.calc_metrics_device(dtype, A.data_ptr(), k, B.data_ptr(), k, mc, n, k, cm["p"].data_ptr(), cm["i"].data_ptr(), cm["nnz"], leg["tp"].data_ptr(),
                                     leg["ti"].data_ptr(), leg["tv"].data_ptr(), mc * t, K, [o.data_ptr() for o in cm["out"]], stream=stream)

    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        for (name, c, t), leg in legs.items():
            ms = timed(lambda: metrics(name, leg, m, leg["out"])); tm = _binding.timings()
            fl = timed(lambda: lists(name, leg)); tf = _binding.timings()
            if keep:
                leg["call_ms"].append(ms); leg["kernel_ms"].append(tm["sweep_ms"]); leg["blocks"] = int(tm["sweep_blocks"])
                leg["floor_ms"].append(fl); leg["floor_kernel_ms"].append(tf["sweep_ms"])
            if name == "NS":
                cm = comps[(c, t)]
                new = timed(lambda: metrics(name, leg, mc, cm["new_out"]))
                old = timed(lambda: complement(c, t))
                if keep:
                    cm["new_ms"].append(new); cm["ms"].append(old)
    torch.cuda.synchronize()
    med = statistics.median
    doc = {"device": torch.cuda.get_device_name(0), "users": m, "k_metrics": K, "dtype": "float32", "reps": args.reps, "warmup": args.warmup, "legs": {},
           "comparison_rm_calc_metrics_dev_f32_on_the_complement": {"users": mc}}
    for (name, c, t), leg in legs.items():
        kernel, floor = med(leg["kernel_ms"]), med(leg["floor_kernel_ms"])
        finite = float(torch.stack([torch.isfinite(o).float().mean() for o in leg["out"]]).min().item())
        doc["legs"]["%s_%d_%d" % (name, c, t)] = {
            "items": items[name][2], "factors": items[name][3], "candidates_per_user": c, "test_items_per_user": t, "kernel_blocks": leg["blocks"],
            "call_ms": [round(x, 4) for x in leg["call_ms"]], "call_median_ms": round(med(leg["call_ms"]), 4),
            "call_spread_ms": round(max(leg["call_ms"]) - min(leg["call_ms"]), 4), "kernel_median_ms": round(kernel, 4),
            "kernel_ns_per_user": round(kernel * 1e6 / m, 1), "finite_share_of_the_worst_output": round(finite, 4),
            "floor_lists_call_median_ms": round(med(leg["floor_ms"]), 4), "floor_lists_kernel_median_ms": round(floor, 4),
            "floor_lists_kernel_ns_per_user": round(floor * 1e6 / m, 1), "kernel_over_floor": round(kernel / floor, 3)}
    ok = True
    for (c, t), cm in comps.items():
        differ = 0
        for a, b in zip(cm["new_out"], cm["out"]):
            differ += int((~((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b)))).sum().item())
        new, spread = med(cm["new_ms"]), max(cm["new_ms"]) - min(cm["new_ms"])
        holds = bool(new + spread < med(cm["ms"]))
        ok = ok and holds and differ == 0
        doc["comparison_rm_calc_metrics_dev_f32_on_the_complement"]["NS_%d_%d" % (c, t)] = {
            "train_entries": cm["nnz"], "complement_call_ms": [round(x, 4) for x in cm["ms"]], "complement_call_median_ms": round(med(cm["ms"]), 4),
            "new_call_ms": [round(x, 4) for x in cm["new_ms"]], "new_call_median_plus_spread_ms": round(new + spread, 4),
            "ratio_complement_over_new": round(med(cm["ms"]) / new, 1), "output_values_that_differ": differ, "condition_holds": holds}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        raise SystemExit("the new call is not below the complement call, or its outputs differ from that call's")


if __name__ == "__main__":
    main()
