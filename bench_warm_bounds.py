#!/usr/bin/env python
"""What model drift keeps of the warm top-K bounds (k_hint_bounds) at BASELINE C2's shape.

    python bench_warm_bounds.py [--baseline-lib PATH] [--reps 7] [--warmup 2] [--out profiles/warm_bounds_drift.json]

A call on the split a context kept seeds its top-K bounds from the lists the call before it left: the K items every user had on its
list are scored with the new factors and the smallest of the K scores is the user's first bound.  bench.py repeats ONE model, the best
case.  This script times rm_calc_metrics_dev_f32 (all ten metrics, inputs resident in HBM, device events around every call) on one
split while the model changes from call to call:

  identical   the same factors every call (bench.py's case)
  eps_1e-3, eps_1e-2, eps_1e-1
              before every call every factor is multiplied by 1 + eps * N(0, 1): the drift of a model between two evaluations, compounding
  unrelated   two models with nothing in common, in turn
  cold        rm_release_workspace() before every call: nothing is kept, every call is a first call

`--baseline-lib`: a librecometrics_hip.so built from the commit to compare with, loaded beside this tree's library; the two are called
in turn on the same sequence of models (which of the two goes first alternates), each on its own context.  Without it the baseline is "not measured".  Per leg and library:
medians (and, for the step, means: a model that does not suit the lists makes the kernel pause, and try again now and then) of `--reps`
calls after `--warmup` -- ms per step, the sweep's and the preparation's stage times (rm_get_timings) -- and the users
that got a warm bound.  The outputs of the two libraries are compared bit for bit after every pair of calls.  One JSON document.

Read the differences with a control: the library the package loads first (this tree's, or RECOMETRICS_HIP_LIB) has measured 0.03-0.09 ms
per call slower than the one loaded with --baseline-lib when both were the SAME build (profiles/warm_bounds_ab_c2.txt section 4) -- run the
script once with a copy of the baseline as RECOMETRICS_HIP_LIB, and once with the roles swapped."""
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
LEGS = ("identical", "eps_1e-3", "eps_1e-2", "eps_1e-1", "unrelated", "cold")
GATED = ("unrelated", "cold")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--users", type=int, default=0, help="fewer users than C2's (quick runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_bounds_drift.json"))
    return ap.parse_args()


def baseline_entry(path):
    """rm_calc_metrics_dev_f32, rm_get_timings and rm_release_workspace of another build of the library"""
    lib = C.CDLL(path)
    vp, i32, i64, u64, sz, ci = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_int
    fn = lib.rm_calc_metrics_dev_f32
    fn.argtypes = [vp, sz, vp, sz, i32, i32, i32, vp, vp, i64, vp, vp, vp, i64, i32, ci, ci] + [vp] * 10 + [ci, i32, i32, u64, vp]
    fn.restype = ci
    lib.rm_last_error.restype = C.c_char_p
    lib.rm_get_timings.argtypes = [C.POINTER(C.c_double), ci]
    lib.rm_get_timings.restype = ci
    lib.rm_release_workspace.restype = ci
    return lib, fn


def main():
    args = parse()
    import torch
    from recometrics_amd import _binding
    from recometrics_amd.synth import CONFIGS, make_factors, make_interactions_fast
    new_lib = _binding.load()
    assert _binding.device_count() > 0, "no HIP device"
    m, n, k, dtype, K, mean_c, seed = CONFIGS["C2"]
    if args.users:
        m = args.users
    trp, tri, tep, tei, tev = make_interactions_fast(m, n, mean_c, dtype, seed)
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    dtrp, dtri, dtep, dtei, dtev = t(trp), t(tri), t(tep), t(tei), t(tev)
    models = [tuple(t(x) for x in make_factors(m, n, k, dtype, seed + i)) for i in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    vp = lambda x: C.c_void_p(int(x)) if x else None                    # noqa: E731
    base = baseline_entry(args.baseline_lib) if args.baseline_lib else None
    libs = (["parent"] if base else []) + ["new"]
    outs = {who: [torch.empty(m, dtype=torch.float32, device=dev) for _ in METRICS] for who in libs}

    entry_of = {"new": baseline_entry(_binding.lib_path())}            # (both libraries through the same raw entry: the same host path)
    if base:
        entry_of["parent"] = base

    def call(who, A, B):
        rc = entry_of[who][1](vp(A.data_ptr()), k, vp(B.data_ptr()), k, m, n, k, vp(dtrp.data_ptr()), vp(dtri.data_ptr()), int(tri.shape[0]),
                     vp(dtep.data_ptr()), vp(dtei.data_ptr()), vp(dtev.data_ptr()), int(tei.shape[0]), K, 0, 0,
                     *[vp(o.data_ptr()) for o in outs[who]], 1, 2, 1, 1, vp(stream))
        if rc:
            raise RuntimeError("%s call failed (%d): %s" % (who, rc, entry_of[who][0].rm_last_error().decode(errors="replace")))

    def timings(who):
        buf = (C.c_double * 12)()
        got = (new_lib if who == "new" else base[0]).rm_get_timings(buf, 12)
        return {"prep_ms": buf[0], "sweep_ms": buf[1], "split_reused": buf[10] if got > 10 else None, "hinted_users": int(buf[11]) if got > 11 else 0}

    def release(who):
        assert (new_lib if who == "new" else base[0]).rm_release_workspace() == 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    doc = {"shape": {"users": m, "items": n, "factors": k, "dtype": np.dtype(dtype).name, "k_metrics": K, "metrics": "all ten"},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "baseline": "library built from the parent commit, called in turn with this tree's" if base else "not measured", "legs": {}}
    equal = True
    for leg in LEGS:
        for who in libs:                                              # every leg starts from nothing kept
            release(who)
        A, B = (x.clone() for x in models[0])
        rows = {who: [] for who in libs}
        for i in range(args.warmup + args.reps):
            if leg.startswith("eps_"):
                eps = float(leg[4:])
                A.mul_(1 + eps * torch.randn(A.shape, generator=gen, device=dev, dtype=A.dtype))
                B.mul_(1 + eps * torch.randn(B.shape, generator=gen, device=dev, dtype=B.dtype))
            elif leg == "unrelated":
                A, B = models[i & 1]
            torch.cuda.synchronize()
            for who in (libs if i % 2 == 0 else libs[::-1]):          # (who goes first takes turns: the second call of a pair finds a warmer device)
                if leg == "cold":
                    release(who)
                ms = timed(lambda: call(who, A, B))
                if i >= args.warmup:
                    rows[who].append(dict(timings(who), ms_per_step=ms))
            if base:
                equal &= all(bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all().item()) for a, b in zip(outs["parent"], outs["new"]))
        med = lambda xs: round(statistics.median(xs), 4)              # noqa: E731
        entry = {}
        for who in libs:
            ms = [r["ms_per_step"] for r in rows[who]]
            entry[who] = {"ms_per_step": med(ms), "ms_per_step_mean": round(statistics.fmean(ms), 4), "hinted_calls": sum(1 for r in rows[who] if r["hinted_users"]),
                          "ms_per_step_min_max": [round(min(ms), 4), round(max(ms), 4)],
                          "sweep_ms": med([r["sweep_ms"] for r in rows[who]]), "prep_ms": med([r["prep_ms"] for r in rows[who]]),
                          "hinted_users": int(statistics.median([r["hinted_users"] for r in rows[who]])),
                          "split_reused": sorted({r["split_reused"] for r in rows[who]}, key=str)}
        if base and leg in GATED:
            spread = entry["parent"]["ms_per_step_min_max"][1] - entry["parent"]["ms_per_step_min_max"][0]
            entry["gate"] = {"rule": "new median <= parent median + the parent's own min-max spread on this leg", "parent_spread_ms": round(spread, 4),
                             "met": bool(entry["new"]["ms_per_step"] <= entry["parent"]["ms_per_step"] + spread)}
        doc["legs"][leg] = entry
        print(leg, json.dumps(entry), flush=True)
    if base:
        doc["outputs_equal_bit_for_bit_in_every_pair"] = bool(equal)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if base and not equal:
        raise SystemExit("the two libraries' outputs differ")
    if base and not all(doc["legs"][leg]["gate"]["met"] for leg in GATED):
        raise SystemExit("a gated leg (unrelated, cold) is slower than the parent by more than the parent's own spread")


if __name__ == "__main__":
    main()
