#!/usr/bin/env python
"""Times the metrics of an item-item model with a sparse W (rm_calc_metrics_item_weights_csr_dev_f32, k_scores_item_weights_csr).

    python bench_item_weights_csr.py [--reps 5] [--warmup 1] [--users 4096] [--out profiles/item_weights_csr.json]

bench_item_weights.py's shape and method: fp32, BASELINE C2's item count, users with MovieLens-like history lengths from
recometrics_amd.synth, the history as the train matrix, all ten metrics, K = 10; inputs resident in HBM, device events around every call,
medians, the legs alternating within every repetition.  W holds 100 stored weights per row at random columns.

  new          the device call on the CSR of W;
  dense        the only route there was: rm_calc_metrics_item_weights_dev_f32 on the same W densified; its ten outputs are compared bit
               for bit with the new call's.  Condition: the new call's median plus its spread (max - min) lies below the dense median;
  kernel       k_scores_item_weights_csr alone (rm_get_timings out[12]), with the bytes of W's (column, weight) pairs it reads (the
               stored entries of the rows the histories name x 8) per second, next to a device-to-device copy of as many bytes.

No hardware counters are collected.  One JSON document."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
K, N_ITEMS, MEAN_C, ROW = 10, 26_744, 144, 100


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--items", type=int, default=N_ITEMS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_weights_csr.json"))
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
    trp, tri, tep, tei, tev = make_interactions_fast(m, n, MEAN_C, dtype, seed=7)
    rng = np.random.default_rng(7)
    hv = rng.uniform(0.5, 5.0, tri.shape[0]).astype(dtype)
    nnz = int(tri.shape[0])
    wp = (np.arange(n + 1) * ROW).astype(np.int32)
    wv = (rng.standard_normal(n * ROW) / ROW ** 0.5).astype(dtype)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_trp, d_tri, d_hv, d_tep, d_tei, d_tev, d_wp, d_wv = (up(a) for a in (trp, tri, hv, tep, tei, tev, wp, wv))
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    # ROW distinct random columns per row, ascending: the places of the smallest ROW of a row of random keys
    d_wi = torch.rand((n, n), generator=gen, device=dev).topk(ROW, dim=1, largest=False).indices.sort(dim=1).values.to(torch.int32).reshape(-1).contiguous()
    wi = d_wi.cpu().numpy()
    W = torch.zeros((n, n), dtype=torch.float32, device=dev)
    W[torch.arange(n, device=dev).repeat_interleave(ROW), d_wi.long()] = d_wv
    outs = {leg: [torch.empty(m, dtype=torch.float32, device=dev) for _ in range(10)] for leg in ("new", "dense")}
    read = int(np.diff(wp)[tri].sum()) * 8                          # (column, weight) pairs of the rows the histories name
    src, dst = torch.empty(read, dtype=torch.uint8, device=dev), torch.empty(read, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    rest = (d_trp.data_ptr(), d_tri.data_ptr(), nnz, d_tep.data_ptr(), d_tei.data_ptr(), d_tev.data_ptr(), int(tei.shape[0]), K)

    def new(out):
        _binding.calc_metrics_item_weights_csr_device(dtype, d_wp.data_ptr(), d_wi.data_ptr(), d_wv.data_ptr(), int(wi.shape[0]), n, m, n,
                                                      d_trp.data_ptr(), d_tri.data_ptr(), d_hv.data_ptr(), nnz, *rest,
                                                      [o.data_ptr() for o in out], stream=stream)

    def old(out):
        _binding.calc_metrics_item_weights_device(dtype, W.data_ptr(), n, n, m, n, d_trp.data_ptr(), d_tri.data_ptr(), d_hv.data_ptr(), nnz, *rest,
                                                  [o.data_ptr() for o in out], stream=stream)

    ms = {leg: [] for leg in ("new", "kernel", "dense", "dense_kernel", "copy")}
    for rep in range(args.warmup + args.reps):
        row = {"new": timed(lambda: new(outs["new"]))}
        row["kernel"] = _binding.item_weights_kernel_ms()
        row["dense"] = timed(lambda: old(outs["dense"]))
        row["dense_kernel"] = _binding.item_weights_kernel_ms()
        row["copy"] = timed(lambda: dst.copy_(src))
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
    doc = {"device": torch.cuda.get_device_name(0), "users": m, "items": n, "history_entries": nnz, "stored_weights_per_row": ROW,
           "k_metrics": K, "dtype": "float32", "reps": args.reps, "warmup": args.warmup, "bytes_of_W_read": read,
           "bytes_of_W_gathered_by_the_dense_route": nnz * n * 4, "finite_share_of_the_worst_output": round(finite, 4),
           "legs": {leg: {"ms": [round(x, 4) for x in v], "median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4)} for leg, v in ms.items()},
           "read_TB_per_s": round(read / (med(ms["kernel"]) * 1e-3) / 1e12, 4),
           "copy_TB_per_s_read_plus_written": round(2 * read / (med(ms["copy"]) * 1e-3) / 1e12, 4),
           "ratio_dense_over_new": round(med(ms["dense"]) / med(ms["new"]), 1), "new_call_median_plus_spread_ms": round(med(ms["new"]) + spread, 4),
           "output_values_that_differ_from_the_dense_route": differ, "hardware_counters": "none collected", "condition_holds": holds}
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
