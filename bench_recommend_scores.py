#!/usr/bin/env python
"""Times the recommendation lists from a caller's score matrix (rm_recommend_scores_dev_f32) at BASELINE C2's shape.

    python bench_recommend_scores.py [--reps 5] [--warmup 1] [--out profiles/recommend_scores_C2.json]

Inputs resident in HBM; S [users x items] is made on the device from C2's synthetic factors (a matrix product; the rows of a
2,048-user stratified sample are then replaced by the library's own k-ordered fma chain, so that for those users rm_recommend_dev_f32
is a bitwise checker).  Device events around every call, the legs alternating within every repetition:

  rowtopk      rm_recommend_scores_dev_f32 at k_top = 10 and 100: the whole call, and from rm_get_timings the row kernel (k_topk_rows:
               reads every row once, selects in LDS) with its achieved bytes/s;
  copy         a plain device-to-device hipMemcpyAsync of the same users x items x 4 bytes -- the yardstick: it reads AND writes what
               the row kernel only reads;
  ascending    rowtopk on the same scores with every row sorted ascending along the item axis: every score beats the bound, the
               buffer is compacted as often as it can be; its ratio to the i.i.d. leg;
  stored_rows  the same calls under RM_DEBUG_NO_ROW_TOPK=1 (k_score_rows -> k_select_topk -> k_finalize_reco), the switch re-read
               and the workspace released between the legs, one untimed call in front of the timed ones.

The lists of the LAST rowtopk call of each k_top are compared with rm_recommend_dev_f32 on the sample, bit for bit.  One JSON document."""
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
K_TOPS = (10, 100)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=0, help="fewer users than C2's (quick runs)")
    ap.add_argument("--sample", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_scores_C2.json"))
    return ap.parse_args()


def stratified_sample(excl_p, m, count, seed=0):
    """the first and the last users, the emptiest and the heaviest exclusion rows, the rest at random"""
    order = np.argsort(np.diff(excl_p), kind="stable")
    edge = min(128, max(1, count // 16))
    pick = set(range(edge)) | set(range(m - edge, m)) | set(order[:edge].tolist()) | set(order[-edge:].tolist())
    for u in np.random.default_rng(seed).permutation(m):
        if len(pick) >= min(count, m):
            break
        pick.add(int(u))
    return np.array(sorted(pick), np.int64)


def main():
    args = parse()
    import torch
    from recometrics_amd import _binding
    from recometrics_amd.synth import CONFIGS, make_factors, make_interactions_fast
    lib = _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    m, n, k, dtype, _, mean_c, seed = CONFIGS["C2"]
    if args.users:
        m = args.users
    A, B = make_factors(m, n, k, dtype, seed)
    trp, tri = make_interactions_fast(m, n, mean_c, dtype, seed)[:2]
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    dA, dB, dtrp, dtri = t(A), t(B), t(trp), t(tri)
    stream = torch.cuda.current_stream().cuda_stream
    # S on the device; the sample's rows by the library's own chain (rm_debug_scores: the sweep's contraction, bit-identical to it)
    dS = dA @ dB.T
    users = stratified_sample(trp, m, args.sample)
    du = torch.from_numpy(users).to(dev)
    dS[du] = t(_binding.debug_scores(A[users], B))
    dAsc = torch.empty_like(dS)
    for a in range(0, m, 8192):                                          # (in pieces: a sort of the whole matrix wants its size again)
        dAsc[a:a + 8192] = torch.sort(dS[a:a + 8192], dim=1).values
    copy_dst = torch.empty_like(dS)
    torch.cuda.synchronize()
    hiprt = C.CDLL("libamdhip64.so")
    hiprt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hiprt.hipMemcpyAsync.restype = C.c_int
    vp = lambda x: C.c_void_p(int(x)) if x else None                    # noqa: E731
    outs = {K: (torch.empty((m, K), dtype=torch.int32, device=dev), torch.empty((m, K), dtype=torch.float32, device=dev),
                torch.empty(m, dtype=torch.int32, device=dev)) for K in K_TOPS}
    scratch = {K: tuple(torch.empty_like(x) for x in outs[K]) for K in K_TOPS}      # (the legs that are not compared)

    def lists(S, K, into):
        _binding.recommend_scores_device(dtype, S.data_ptr(), n, m, n, dtrp.data_ptr(), dtri.data_ptr(), int(tri.shape[0]), K,
                                         into[0].data_ptr(), into[1].data_ptr(), into[2].data_ptr(), stream)

    def copy():
        rc = hiprt.hipMemcpyAsync(vp(copy_dst.data_ptr()), vp(dS.data_ptr()), m * n * 4, 3, vp(stream))      # 3 = device to device
        if rc:
            raise RuntimeError("hipMemcpyAsync failed (%d)" % rc)

    def stored_rows(on):
        """the switch, read again, with the workspace released: the next call allocates what its path needs and nothing else"""
        torch.cuda.synchronize()
        if on:
            os.environ["RM_DEBUG_NO_ROW_TOPK"] = "1"
        else:
            os.environ.pop("RM_DEBUG_NO_ROW_TOPK", None)
        _binding.reload_switches()
        assert lib.rm_release_workspace() == 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    keys = ("prep_ms", "sweep_ms", "finalize_ms", "device_ms", "sweep_blocks")
    t_row = {K: [] for K in K_TOPS}; t_asc = {K: [] for K in K_TOPS}; t_sto = {K: [] for K in K_TOPS}
    s_row = {K: [] for K in K_TOPS}; s_asc = {K: [] for K in K_TOPS}; s_sto = {K: [] for K in K_TOPS}
    t_copy = []
    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        stored_rows(False)
        lists(dS, K_TOPS[0], scratch[K_TOPS[0]])                        # (untimed: the workspace of this path)
        for K in K_TOPS:
            ms = timed(lambda: lists(dS, K, outs[K])); tm = _binding.timings()
            if keep:
                t_row[K].append(ms); s_row[K].append({key: tm[key] for key in keys})
            ms = timed(copy)
            if keep:
                t_copy.append(ms)
            ms = timed(lambda: lists(dAsc, K, scratch[K])); tm = _binding.timings()
            if keep:
                t_asc[K].append(ms); s_asc[K].append({key: tm[key] for key in keys})
        stored_rows(True)
        lists(dS, K_TOPS[0], scratch[K_TOPS[0]])
        for K in K_TOPS:
            ms = timed(lambda: lists(dS, K, scratch[K])); tm = _binding.timings()
            if keep:
                t_sto[K].append(ms); s_sto[K].append({key: tm[key] for key in keys})
    stored_rows(False)
    # the lists of the last rowtopk calls against the factor call, on the sample, bit for bit
    parity = {}
    sA = dA[du].contiguous()
    sp = np.zeros(users.shape[0] + 1, np.int64)
    np.cumsum(np.diff(trp)[users], out=sp[1:])
    si = np.concatenate([tri[trp[u]:trp[u + 1]] for u in users]) if users.shape[0] else np.zeros(0, np.int32)
    dsp, dsi = t(sp.astype(np.int32)), t(si.astype(np.int32))
    for K in K_TOPS:
        fi = torch.empty((users.shape[0], K), dtype=torch.int32, device=dev)
        fs = torch.empty((users.shape[0], K), dtype=torch.float32, device=dev)
        ft = torch.empty(users.shape[0], dtype=torch.int32, device=dev)
        _binding.recommend_device(dtype, sA.data_ptr(), k, dB.data_ptr(), k, int(users.shape[0]), n, k, dsp.data_ptr(), dsi.data_ptr(), int(si.shape[0]), K,
                                  fi.data_ptr(), fs.data_ptr(), ft.data_ptr(), stream)
        torch.cuda.synchronize()
        gi, gs, gt = (x[du] for x in outs[K])
        same_s = (gs.view(torch.int32) == fs.view(torch.int32)) | (torch.isnan(gs) & torch.isnan(fs))
        parity[str(K)] = {"users_checked": int(users.shape[0]), "ids_differ": int((gi != fi).sum().item()), "scores_differ": int((~same_s).sum().item()),
                          "status_differ": int((gt != ft).sum().item())}
        parity[str(K)]["bit_equal"] = not (parity[str(K)]["ids_differ"] or parity[str(K)]["scores_differ"] or parity[str(K)]["status_differ"])
    med = statistics.median
    copy_ms = med(t_copy)
    read_bytes = m * n * 4

    def leg(ts, ss):
        kernel_ms = med([s["sweep_ms"] for s in ss])
        return {"call_ms": [round(x, 4) for x in ts], "call_median_ms": round(med(ts), 4),
                "timings_median_ms": {key: round(med([s[key] for s in ss]), 4) for key in keys[:4]},
                "row_kernel_blocks": int(ss[-1]["sweep_blocks"]), "row_kernel_median_ms": round(kernel_ms, 4)}

    doc = {"shape": {"users": m, "items": n, "dtype": np.dtype(dtype).name, "k_top": list(K_TOPS), "nnz_excl": int(tri.shape[0]),
                     "score_matrix_bytes": read_bytes},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "copy_yardstick": {"what": "hipMemcpyAsync device to device, users x items x 4 bytes", "bytes_read_and_written": 2 * read_bytes,
                              "ms": [round(x, 4) for x in t_copy], "median_ms": round(copy_ms, 4),
                              "achieved_bytes_per_s": round(2 * read_bytes / (copy_ms * 1e-3))},
           "rowtopk": {}, "ascending": {}, "stored_rows": {}, "parity_vs_rm_recommend_dev": parity}
    for K in K_TOPS:
        r = leg(t_row[K], s_row[K])
        r["row_kernel_bytes_read"] = read_bytes
        r["row_kernel_achieved_bytes_per_s"] = round(read_bytes / (r["row_kernel_median_ms"] * 1e-3)) if r["row_kernel_median_ms"] > 0 else None
        r["row_kernel_over_copy"] = round(r["row_kernel_median_ms"] / copy_ms, 4)
        doc["rowtopk"][str(K)] = r
        a = leg(t_asc[K], s_asc[K])
        a["row_kernel_over_iid"] = round(a["row_kernel_median_ms"] / r["row_kernel_median_ms"], 4) if r["row_kernel_median_ms"] > 0 else None
        doc["ascending"][str(K)] = a
        s = leg(t_sto[K], s_sto[K])
        s["call_over_rowtopk_call"] = round(s["call_median_ms"] / r["call_median_ms"], 4)
        doc["stored_rows"][str(K)] = s
    doc["target_row_kernel_k10_at_most_copy"] = bool(doc["rowtopk"]["10"]["row_kernel_median_ms"] <= copy_ms)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not all(p["bit_equal"] for p in parity.values()):
        raise SystemExit("the timed lists differ from rm_recommend_dev_f32's on the sample")


if __name__ == "__main__":
    main()
