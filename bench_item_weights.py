#!/usr/bin/env python
"""Times the metrics of an item-item model (rm_calc_metrics_item_weights_dev_f32, k_scores_item_weights).

    python bench_item_weights.py [--reps 5] [--warmup 1] [--users 4096] [--out profiles/item_weights.json]

fp32, BASELINE C2's item count (W 26,744 x 26,744), users with MovieLens-like history lengths from recometrics_amd.synth (lognormal, mean
about 100 stored entries, non-integer values), the history as the train matrix, all ten metrics, K = 10.  Inputs resident in HBM, device
events around every call, medians, the legs alternating within every repetition:

  new          the device call;
  dense        the route there was: rm_calc_metrics_dev_f32 on dense(X_hist) and W^T, the same users; its ten outputs are compared bit
               for bit with the new call's.  Condition: the new call's median plus its spread (max - min) lies below the dense median;
  kernel       k_scores_item_weights alone (rm_get_timings out[12]), with the bytes of W it gathers (nnz_hist x n x 4) per second,
               next to a device-to-device copy of as many bytes (2 GiB pieces, read + written).

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
K, N_ITEMS, MEAN_C = 10, 26_744, 144


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--items", type=int, default=N_ITEMS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_weights.json"))
    return ap.parse_args()


def main():
    args = parse()
    import torch
    from recometrics_amd import _binding
    from recometrics_amd.synth import make_interactions_fast
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    assert args.reps >= 5, "medians of at least five calls"
    dev, m, n, dtype = torch.device("cuda:0"), args.users, args.items, np.float32
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    trp, tri, tep, tei, tev = make_interactions_fast(m, n, MEAN_C, dtype, seed=7)
    hv = np.random.default_rng(7).uniform(0.5, 5.0, tri.shape[0]).astype(dtype)
    nnz = int(tri.shape[0])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_trp, d_tri, d_hv, d_tep, d_tei, d_tev = (up(a) for a in (trp, tri, hv, tep, tei, tev))
    W = torch.randn((n, n), generator=gen, device=dev) / n ** 0.5
    Wt = W.t().contiguous()
    dense = torch.zeros((m, n), dtype=torch.float32, device=dev)
    dense[torch.repeat_interleave(torch.arange(m, device=dev), up(np.diff(trp)).long()), d_tri.long()] = d_hv
    outs = {leg: [torch.empty(m, dtype=torch.float32, device=dev) for _ in range(10)] for leg in ("new", "dense")}
    piece = min(nnz * n * 4, 2 << 30)
    src, dst = torch.empty(piece, dtype=torch.uint8, device=dev), torch.empty(piece, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def new(out):
        _binding.calc_metrics_item_weights_device(dtype, W.data_ptr(), n, n, m, n, d_trp.data_ptr(), d_tri.data_ptr(), d_hv.data_ptr(), nnz,
                                                  d_trp.data_ptr(), d_tri.data_ptr(), nnz, d_tep.data_ptr(), d_tei.data_ptr(), d_tev.data_ptr(),
                                                  int(tei.shape[0]), K, [o.data_ptr() for o in out], stream=stream)

    def old(out):
        _binding.calc_metrics_device(dtype, dense.data_ptr(), n, Wt.data_ptr(), n, m, n, n, d_trp.data_ptr(), d_tri.data_ptr(), nnz, d_tep.data_ptr(),
                                     d_tei.data_ptr(), d_tev.data_ptr(), int(tei.shape[0]), K, [o.data_ptr() for o in out], stream=stream)

    def copy():
        left = nnz * n * 4
        while left > 0:
            dst[:min(left, piece)].copy_(src[:min(left, piece)])
            left -= piece

    ms = {leg: [] for leg in ("new", "dense", "copy", "kernel")}
    for rep in range(args.warmup + args.reps):
        row = {"new": timed(lambda: new(outs["new"]))}
        row["kernel"] = _binding.item_weights_kernel_ms()
        row["dense"] = timed(lambda: old(outs["dense"]))
        row["copy"] = timed(copy)
        if rep >= args.warmup:
            for leg, x in row.items():
                ms[leg].append(x)
    torch.cuda.synchronize()
    med = statistics.median
    differ = sum(int((~((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b)))).sum().item())
                 for a, b in zip(outs["new"], outs["dense"]))
    finite = float(torch.stack([torch.isfinite(o).float().mean() for o in outs["dense"]]).min().item())
    spread = max(ms["new"]) - min(ms["new"])
    holds = bool(med(ms["new"]) + spread < med(ms["dense"]))
    gathered = nnz * n * 4
    doc = {"device": torch.cuda.get_device_name(0), "users": m, "items": n, "history_entries": nnz, "k_metrics": K, "dtype": "float32",
           "reps": args.reps, "warmup": args.warmup, "gathered_bytes": gathered, "finite_share_of_the_worst_output": round(finite, 4),
           "legs": {leg: {"ms": [round(x, 4) for x in v], "median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4)} for leg, v in ms.items()},
           "gathered_TB_per_s": round(gathered / (med(ms["kernel"]) * 1e-3) / 1e12, 3),
           "copy_TB_per_s_read_plus_written": round(2 * gathered / (med(ms["copy"]) * 1e-3) / 1e12, 3),
           "ratio_dense_over_new": round(med(ms["dense"]) / med(ms["new"]), 1), "new_call_median_plus_spread_ms": round(med(ms["new"]) + spread, 4),
           "output_values_that_differ_from_the_dense_route": differ, "condition_holds": holds}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not (holds and differ == 0):
        raise SystemExit("the new call is not below the dense route, or its outputs differ from that route's")


if __name__ == "__main__":
    main()
