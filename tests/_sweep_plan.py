"""One visit per row of the two tables of sweep-kernel instantiations (csrc/rm_sweep_units.hip), written as data.

Pure Python: nothing here is imported from the product.  tests/test_sweep_coverage_cpu.py checks the plan against the table
without a GPU; tests/test_hip_sweep_rows.py walks it on one, with the library's launch ledger (rm_debug_sweep_launched) as the
proof of which row every call ran.

A visit is a call -- factor count, k_metrics, request, RM_* switches -- and the key it must launch.  The call of a row comes from
`_recipe` (the row read backwards: which call reaches it); the key of a call from `predict_key`, a restatement of the pipeline's
choice (csrc/rm_lib.hip: Prec::supported_ng, lane_lists_possible, plan_stage's ext_topk, sweep_geometry's nsub and list_in_lds,
set_spec, dispatch_sweep; csrc/rm_sweep_units.hip: sweep_key).  A recipe that does not lead back to its row shows as a row without
a primary visit.

What the restatement takes from the problem the visits run on (tests/test_hip_sweep_rows.py builds it so; the ledger says where
not): every score finite by the bound on the factors (check_nan 0), no tie noise, a catalogue small enough for the dense train rows
and too small for a sample seed, lane buffers that fit the device's memory, test rows of at most 63 items outside the streamed
users (tables of depth JMAX)."""
import collections

from test_sweep_table_cpu import LM_APPEND, LM_HBM, LM_LDS, expected_units

ALL = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr")
TOPK8 = ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr")            # (= tests/_requests.py TOPK8: no ROC / PR-AUC, the auc = 0 kernels)
K_LDS, K_HBM, K_APPEND = 5, 7, 40
SPLITS = {"RM_DEBUG_SPLITS": "2,1,3"}                                 # every metric visit: two item ranges, a tail level of three
SWITCHES = ("RM_DEBUG_SPLITS", "RM_DEBUG_HBM_LISTS", "RM_DEBUG_NSUB2", "RM_DEBUG_NO_TRAIN_BITS", "RM_DEBUG_NO_SPEC", "RM_DEBUG_EXT_TOPK",
            "RM_DEBUG_LANE_MIN_K")
RUNTIME_FACTORS = {"f32": 637, "f64": 517}                            # ng 0: 80 groups = five 16-group chunks / 72 groups = nine 8-group chunks
DUMP_SHAPE = {"f32": (70, 333), "f64": (37, 150)}                     # debug_scores problems (users, items)
LDS_LIMIT, SYNC_BYTES, JMAX = 160 * 1024, 32, 6
COMPILED_NG = {"f32": (2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16, 32, 64), "f64": (2, 3, 4, 5, 6, 7, 8, 16, 32, 64)}

Visit = collections.namedtuple("Visit", "prec unit kind factors K request env key primary")
# kind "metric": hip_calc(request, K, cumulative) under env; kind "dump": debug_scores at DUMP_SHAPE.  primary: the row's one visit.

# Rows no entry point reaches, as (prec, key, "file:line that proves it").  None found: every row below has its call.
UNREACHABLE = []


def factors_of(prec, ng):
    """the factor count a row is visited at: the last group of 8 ragged; the run-time kernel at whole chunks"""
    return RUNTIME_FACTORS[prec] if ng == 0 else 8 * ng - 3


def supported_ng(prec, factors):
    """Prec::supported_ng: the smallest compiled group count that holds the factors, beyond those whole chunks (16 / 8 groups)"""
    ng = max(1, (factors + 7) // 8)
    for have in COMPILED_NG[prec]:
        if ng <= have:
            return have
    chunk = 16 if prec == "f32" else 8
    return (ng + chunk - 1) // chunk * chunk


def sweep_lds(prec, ng, K, auc, with_lists, nsub, j):
    """sweep_lds: the operand tiles, the lists, and -- with the AUCs -- four groups' positives tables of 2^j rows"""
    if prec == "f32":
        gu, elem = 32, 4
        head = 2 * min(ng, 16) * 2 * (32 * nsub) * 16 + (4 * (K + 2) * gu * 8 if with_lists else 0)
    else:
        gu, elem = 16, 8
        head = 2 * min(ng, 8) * 4 * 64 * 16 + (4 * nsub * K * gu * 16 if with_lists else 0)
    if not auc:
        return head
    tb = (1 << j) * gu * elem
    return (head + tb - 1) // tb * tb + 4 * (1 << j) * gu * (elem + 4)


def predict_choice(prec, factors, K, auc, env):
    """(ng, lmode, nsub, spec) the pipeline asks dispatch_sweep for"""
    ng = supported_ng(prec, factors)
    three = prec == "f32" and ng <= 8                                  # the lists' kernel would run three sub-tiles
    min_k = int(env["RM_DEBUG_LANE_MIN_K"]) if "RM_DEBUG_LANE_MIN_K" in env else (20 if three else 1 if prec == "f64" else 14)
    forced_ext = "RM_DEBUG_EXT_TOPK" in env
    lane = not forced_ext and min_k <= K <= 1354                       # lane_lists_possible (K + a lane buffer <= 4,096 entries)
    ext_topk = forced_ext or (not lane and K > 256)
    hbm = "RM_DEBUG_HBM_LISTS" in env
    j = JMAX if auc else 0

    def fits(nsub):
        return sweep_lds(prec, ng, K, auc, True, nsub, j) + SYNC_BYTES <= LDS_LIMIT
    lists = not ext_topk and not lane
    nsub = 3 if lists and three and fits(3) and not hbm and "RM_DEBUG_NSUB2" not in env else 2
    lmode = LM_LDS if lists and fits(nsub) and not hbm else LM_APPEND if lane or ext_topk else LM_HBM
    if ext_topk or "RM_DEBUG_NO_SPEC" in env:
        spec = 0
    else:
        spec = 1 if prec == "f64" or "RM_DEBUG_NO_TRAIN_BITS" not in env else 2
    return ng, lmode, nsub, spec


def sweep_key(prec, ng, auc, dump, lmode, nsub, spec):
    """sweep_key for a call packed for its own group count (ngt = ng)"""
    chunk = 16 if prec == "f32" else 8
    tng = 0 if ng > 64 and ng % chunk == 0 else ng
    if prec == "f32":
        if nsub == 3:
            return (ng, int(auc), 0, LM_LDS, 3, spec)
        if ng > 16:
            spec = 0
    else:
        nsub, spec = 2, int(spec == 1)
    return (tng, 0, 1, LM_HBM, 2, 0) if dump else (tng, int(auc), 0, lmode, 2, spec)


def predict_key(prec, factors, K, auc, env, dump=False):
    if dump:                                                           # debug_scores: dispatch_sweep(false, true, false, 2, ...), spec 0
        return sweep_key(prec, supported_ng(prec, factors), False, True, LM_HBM, 2, 0)
    ng, lmode, nsub, spec = predict_choice(prec, factors, K, auc, env)
    return sweep_key(prec, ng, auc, False, lmode, nsub, spec)


def _recipe(prec, row):
    """the call that reaches `row`: (K, request, env)"""
    ng, auc, dump, lmode, nsub, spec = row
    env = dict(SPLITS)
    K = {LM_LDS: K_LDS, LM_HBM: K_HBM, LM_APPEND: K_APPEND}[lmode]
    if lmode == LM_HBM:
        env["RM_DEBUG_HBM_LISTS"] = "1"
    if prec == "f64" and lmode != LM_APPEND:                           # fp64 takes the lane buffers at every K
        env["RM_DEBUG_LANE_MIN_K"] = "1000000"
    if prec == "f32" and lmode == LM_LDS and nsub == 2 and 0 < ng <= 8:
        env["RM_DEBUG_NSUB2"] = "1"
    compiled_spec = prec == "f64" or 0 < ng <= 16                      # (fp32 beyond 128 factors: the key says 0 whatever the call asks for)
    if compiled_spec and spec == 0:
        env["RM_DEBUG_NO_SPEC"] = "1"
    if compiled_spec and spec == 2:
        env["RM_DEBUG_NO_TRAIN_BITS"] = "1"
    return K, (ALL if auc else TOPK8), env


def _visits():
    out = []
    for prec, units in expected_units().items():
        for unit, rows in units.items():
            for row in rows:
                ng, auc, dump, lmode, nsub, spec = row
                factors = factors_of(prec, ng)
                if dump:
                    out.append(Visit(prec, unit, "dump", factors, 0, (), {}, predict_key(prec, factors, 0, False, {}, dump=True), True))
                    continue
                K, request, env = _recipe(prec, row)

                def visit(env, primary):
                    return Visit(prec, unit, "metric", factors, K, request, env, predict_key(prec, factors, K, bool(auc), env), primary)
                out.append(visit(env, True))
                # second visits: the SPEC 0 kernels read their switches at run time
                if spec == 0 and prec == "f32" and 0 < ng <= 16:       # the CSR cursor instead of the dense train rows
                    out.append(visit(dict(env, RM_DEBUG_NO_TRAIN_BITS="1"), False))
                if spec == 0 and lmode == LM_APPEND:                   # sa.ext_topk = 1: every lane streams, k_select_topk picks
                    ext = {k: v for k, v in env.items() if k != "RM_DEBUG_NO_SPEC"}
                    out.append(visit(dict(ext, RM_DEBUG_EXT_TOPK="1"), False))
    return out


VISITS = _visits()


def visits_of(prec, unit):
    return [v for v in VISITS if v.prec == prec and v.unit == unit]


def unit_ids():
    return [(prec, unit) for prec, units in expected_units().items() for unit in units]
