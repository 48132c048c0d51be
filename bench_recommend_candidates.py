#!/usr/bin/env python
"""Times the lists from per-user candidate sets (rm_recommend_candidates_dev_f32, k_topk_candidates).

    python bench_recommend_candidates.py [--reps 5] [--warmup 1] [--out profiles/recommend_candidates.json]

fp32, inputs resident in HBM, device events around every call, medians, the legs alternating within every repetition.  Item matrices:
BASELINE C2's (26,744 x 64) and the north star's (1,000,000 x 128); 16,384 users; 128 and 1,024 uniformly drawn candidates per user
(a draw may repeat an id: it counts once); k_top = 10.  Per leg: ms per call and for the kernel alone (rm_get_timings), candidate rows
per second, gathered bytes per second (entries x k x 4 over the kernel's time), and next to it a device-to-device hipMemcpyAsync of the
same byte count, measured in the same repetitions -- the yardstick reads AND writes contiguous memory, the kernel gathers rows.

  self-check   on the C2 matrix the candidate rows of a few users (--sample, spread over the range) are the WHOLE catalogue; their lists
               from the last timed call of each leg are compared, bit for bit, with rm_recommend_dev_f32 without an exclusion matrix.
               (Their rows are part of what is timed and counted: entries, not users x candidates, are what the rates divide.)
  comparison   the only other route to such lists: rm_recommend_dev_f32 over the whole 1 M catalogue for the same users, nothing excluded.
               Condition: at 1,024 candidates the new call's median plus its own spread (max - min) lies below that leg's median.

One JSON document."""
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
K_TOP = 10
CATALOGUES = (("C2", 26_744, 64), ("NS", 1_000_000, 128))
CANDIDATES = (128, 1024)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=16384)
    ap.add_argument("--sample", type=int, default=8, help="users of the C2 legs whose candidate row is the whole catalogue")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_candidates.json"))
    return ap.parse_args()


def main():
    args = parse()
    import torch
    from recometrics_amd import _binding
    _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    assert args.reps >= 5, "medians of at least five calls"
    dev, m, dtype = torch.device("cuda:0"), args.users, np.float32
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    hiprt = C.CDLL("libamdhip64.so")
    hiprt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hiprt.hipMemcpyAsync.restype = C.c_int

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def outputs(users):
        return (torch.empty((users, K_TOP), dtype=torch.int32, device=dev), torch.empty((users, K_TOP), dtype=torch.float32, device=dev),
                torch.empty(users, dtype=torch.int32, device=dev))

    # the problems: factors, and per leg the candidate CSR (rows sorted; the sample's rows replaced by the whole catalogue)
    legs, items = {}, {}
    sample = np.linspace(0, m - 1, args.sample).round().astype(np.int64) if args.sample else np.zeros(0, np.int64)
    for name, n, k in CATALOGUES:
        A = torch.randn((m, k), generator=gen, device=dev) / k ** 0.5
        B = torch.randn((n, k), generator=gen, device=dev) / k ** 0.5
        items[name] = (A, B, n, k)
        for c in CANDIDATES:
            rows = torch.sort(torch.randint(n, (m, c), generator=gen, device=dev, dtype=torch.int32), dim=1).values
            lens = torch.full((m,), c, dtype=torch.int64, device=dev)
            whole = torch.from_numpy(sample).to(dev) if name == "C2" else torch.zeros(0, dtype=torch.int64, device=dev)
            lens[whole] = n
            p = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            p[1:] = torch.cumsum(lens, 0)
            nnz = int(p[-1].item())
            i = torch.empty(nnz, dtype=torch.int32, device=dev)
            plain = torch.ones(m, dtype=torch.bool, device=dev)
            plain[whole] = False
            at = (p[:-1][plain].unsqueeze(1) + torch.arange(c, device=dev).unsqueeze(0)).reshape(-1)
            i[at] = rows[plain].reshape(-1)
            for u in whole.tolist():
                i[int(p[u].item()):int(p[u + 1].item())] = torch.arange(n, dtype=torch.int32, device=dev)
            legs[(name, c)] = {"p": p.to(torch.int32), "i": i, "nnz": nnz, "out": outputs(m), "call_ms": [], "kernel_ms": [], "copy_ms": [], "blocks": 0}
    most = max(leg["nnz"] * items[name][3] * 4 for (name, _), leg in legs.items())
    copy_src, copy_dst = (torch.empty(most, dtype=torch.uint8, device=dev) for _ in range(2))
    full_out, t_full = outputs(m), []
    torch.cuda.synchronize()

    def candidates(name, c):
        A, B, n, k = items[name]
        leg = legs[(name, c)]
        _binding.recommend_candidates_device(dtype, A.data_ptr(), k, B.data_ptr(), k, m, n, k, leg["p"].data_ptr(), leg["i"].data_ptr(), leg["nnz"], K_TOP,
                                             leg["out"][0].data_ptr(), leg["out"][1].data_ptr(), leg["out"][2].data_ptr(), stream)

    def copy(nbytes):
        rc = hiprt.hipMemcpyAsync(C.c_void_p(copy_dst.data_ptr()), C.c_void_p(copy_src.data_ptr()), nbytes, 3, C.c_void_p(stream) if stream else None)      # 3 = device to device
        if rc:
            raise RuntimeError("hipMemcpyAsync failed (%d)" % rc)

    def full_catalogue(name, A, out):
        _, B, n, k = items[name]
        _binding.recommend_device(dtype, A.data_ptr(), k, B.data_ptr(), k, int(A.shape[0]), n, k, 0, 0, 0, K_TOP, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream)

    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        for (name, c), leg in legs.items():
            ms = timed(lambda: candidates(name, c)); tm = _binding.timings()
            cp = timed(lambda: copy(leg["nnz"] * items[name][3] * 4))
            if keep:
                leg["call_ms"].append(ms); leg["kernel_ms"].append(tm["sweep_ms"]); leg["copy_ms"].append(cp); leg["blocks"] = int(tm["sweep_blocks"])
            if (name, c) == ("NS", 1024):                               # (the comparison leg, right behind the leg it is compared with)
                ms = timed(lambda: full_catalogue("NS", items["NS"][0], full_out))
                if keep:
                    t_full.append(ms)
    # the self-check: the whole-catalogue rows of the last timed C2 calls against rm_recommend_dev_f32, nothing excluded
    parity = {}
    if sample.shape[0]:
        du = torch.from_numpy(sample).to(dev)
        want = outputs(sample.shape[0])
        full_catalogue("C2", items["C2"][0][du].contiguous(), want)
        torch.cuda.synchronize()
        for c in CANDIDATES:
            gi, gs, gt = (x[du] for x in legs[("C2", c)]["out"])
            same_s = (gs.view(torch.int32) == want[1].view(torch.int32)) | (torch.isnan(gs) & torch.isnan(want[1]))
            parity[str(c)] = {"users_checked": int(sample.shape[0]), "ids_differ": int((gi != want[0]).sum().item()),
                              "scores_differ": int((~same_s).sum().item()), "status_differ": int((gt != want[2]).sum().item())}
            parity[str(c)]["bit_equal"] = not (parity[str(c)]["ids_differ"] or parity[str(c)]["scores_differ"] or parity[str(c)]["status_differ"])
    med = statistics.median
    doc = {"device": torch.cuda.get_device_name(0), "users": m, "k_top": K_TOP, "dtype": "float32", "reps": args.reps, "warmup": args.warmup,
           "whole_catalogue_rows_in_the_C2_legs": int(sample.shape[0]), "legs": {}, "self_check_vs_rm_recommend_dev_f32": parity}
    for (name, c), leg in legs.items():
        _, _, n, k = items[name]
        nbytes, kernel, cp = leg["nnz"] * k * 4, med(leg["kernel_ms"]), med(leg["copy_ms"])
        doc["legs"]["%s_%d" % (name, c)] = {
            "items": n, "factors": k, "candidates_per_user": c, "entries": leg["nnz"], "gathered_bytes": nbytes, "kernel_blocks": leg["blocks"],
            "call_ms": [round(x, 4) for x in leg["call_ms"]], "call_median_ms": round(med(leg["call_ms"]), 4),
            "call_spread_ms": round(max(leg["call_ms"]) - min(leg["call_ms"]), 4), "kernel_median_ms": round(kernel, 4),
            "candidate_rows_per_s": round(leg["nnz"] / (kernel * 1e-3)), "gathered_bytes_per_s": round(nbytes / (kernel * 1e-3)),
            "copy_same_bytes_median_ms": round(cp, 4), "copy_bytes_per_s_read_plus_written": round(2 * nbytes / (cp * 1e-3)),
            "kernel_over_copy": round(kernel / cp, 4)}
    new = doc["legs"]["NS_1024"]
    doc["comparison_rm_recommend_dev_f32_whole_NS_catalogue"] = {
        "call_ms": [round(x, 4) for x in t_full], "call_median_ms": round(med(t_full), 4),
        "new_call_median_plus_spread_ms": round(new["call_median_ms"] + new["call_spread_ms"], 4),
        "ratio_comparison_over_new": round(med(t_full) / new["call_median_ms"], 2),
        "condition_holds": bool(new["call_median_ms"] + new["call_spread_ms"] < med(t_full))}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not all(p["bit_equal"] for p in parity.values()):
        raise SystemExit("the timed lists differ from rm_recommend_dev_f32's on the sample")
    if not doc["comparison_rm_recommend_dev_f32_whole_NS_catalogue"]["condition_holds"]:
        raise SystemExit("the new call is not below the whole-catalogue call")


if __name__ == "__main__":
    main()
