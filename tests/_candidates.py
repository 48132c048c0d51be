"""Candidate rows, ordered factors and a model of k_topk_candidates' schedule, for tests/test_hip_candidates.py,
tests/test_hip_candidates_structured.py (GPU) and tests/test_candidates_structured_cpu.py (which proves, without a GPU, that the
rows of the GPU module reach the branches they are meant for).  Pure NumPy; of the product only recometrics_amd.synth is imported.

schedule() is a model of what the comment at the head of csrc/rm_candidates.hpp promises -- steps, duplicates, the compaction in
front of a step that could overflow the buffer, the bound -- written from that comment, not from the kernel's code."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64

# the three numbers schedule() restates
CAND_STEP = 256          # csrc/rm_candidates.hpp: `constexpr int CAND_STEP = SCORE_ROW_THREADS;` (csrc/rm_scores.hpp: 256): entries per step
WAVE = 64                # csrc/rm_candidates.hpp, "Geometry": "256 consecutive entries of the row, 64 per wavefront, one per lane"
CAP = 2048               # csrc/rm_rowtopk.hpp: `constexpr int ROW_TOPK_CAP = 2048;`: pairs of the append buffer; longer rows compact


# ---- CSR helpers ----------------------------------------------------------------------------------------------------------------
def csr_of(rows):
    p = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=p[1:])
    return p.astype(np.int32), np.concatenate(rows).astype(np.int32)


def rows_of(cand):
    return [cand[1][cand[0][u]:cand[0][u + 1]] for u in range(cand[0].shape[0] - 1)]


def complement_of(cand, n):
    return csr_of([np.setdiff1d(np.arange(n, dtype=np.int32), r) for r in rows_of(cand)])


def spread_rows(counts, n, seed):
    """sorted rows of `counts` distinct ids over the whole id range, ids 0 and n - 1 among them wherever there are two or more"""
    rng = np.random.default_rng(seed)
    return csr_of([np.sort(np.concatenate([rng.choice(np.arange(1, n - 1), max(c - 2, 0), replace=False), [0, n - 1][:min(c, 2)]])) for c in counts])


def shuffled(cand, seed):
    """every row in an order of its own"""
    rng = np.random.default_rng(seed)
    return csr_of([rng.permutation(r) for r in rows_of(cand)])


# ---- factors --------------------------------------------------------------------------------------------------------------------
BLOCK = 300                                                          # item rows per block of `blocks`
STRUCTURED = ("ascending", "descending", "trend", "runs", "blocks", "equal")


def _no_interactions(m, n, mean_c, dtype, seed, test_fraction):
    z = np.zeros(m + 1, np.int32)
    return z, np.zeros(0, np.int32), z.copy(), np.zeros(0, np.int32), np.zeros(0, dtype)


def structured_factors(kind, m, n, kf, dtype, seed):
    """(A, B) whose scores follow the item id: ascending / descending / trend / runs are synth.make_structured's; `blocks` is the
    ascending ramp with every BLOCK consecutive item rows identical (later blocks better); `equal` has one item row for everybody;
    `iid` is synth.make_factors (the control)."""
    from recometrics_amd.synth import make_factors, make_structured
    if kind == "iid":
        return make_factors(m, n, kf, dtype, seed)
    pr = make_structured("ascending" if kind in ("blocks", "equal") else kind, m, n, kf, dtype, seed=seed, interactions=_no_interactions)
    A, B = pr["A"], pr["B"]
    if kind == "blocks":
        B = np.ascontiguousarray(B[np.arange(n) // BLOCK * BLOCK])
    elif kind == "equal":
        B = np.ascontiguousarray(B[np.full(n, n // 3)])
    return A, B


# ---- rows -----------------------------------------------------------------------------------------------------------------------
def dup_run(base_row, at, times):
    """the distinct sorted row with the id at position `at` standing `times` times in all"""
    base_row = np.asarray(base_row)
    assert (np.diff(base_row) > 0).all() and 0 <= at < base_row.shape[0] and times >= 1
    return np.concatenate([base_row[:at], np.full(times, base_row[at], base_row.dtype), base_row[at + 1:]])


def few_distinct(n, entries, distinct, rng):
    """a sorted row of `entries` entries that holds `distinct` different ids of [0, n), each at least once"""
    ids = rng.choice(n, distinct, replace=False)
    return np.sort(np.concatenate([ids, rng.choice(ids, entries - distinct)])).astype(np.int32)


def chained(rows):
    """sorted rows; row u + 1 begins with the last id of row u (what lies below it is dropped), and every row ends with 70 entries
    of its last id"""
    out, last = [], None
    for r in rows:
        r = np.asarray(r)
        assert (np.diff(r) > 0).all()
        if last is not None:
            r = np.concatenate([[last], r[r > last]])
        assert r.shape[0] >= 2, "nothing left above the previous row's last id"
        last = r[-1]
        out.append(dup_run(r, r.shape[0] - 1, 70).astype(np.int32))
    return out


# ---- the schedule of k_topk_candidates ------------------------------------------------------------------------------------------
def schedule(ids_row, scores_row, K):
    """What the kernel does with a SORTED row of entries `ids_row` whose scores are scores_row[id], as a dict:

    longrow          more than CAP entries: the row compacts and keeps a bound
    live             entries that differ from their predecessor (the distinct ids)
    compactions      sorts in front of a step with count + CAND_STEP > CAP
    appends          pairs appended in all; appends_after: those behind the first compaction
    idle             (wavefront, step) cells inside the row none of whose entries is live
    idle_then_live   idle cells whose wavefront has a live entry in the next step; live_then_idle: ... in the previous step
    idle_steps       steps none of whose entries is live
    bound_in_tie     a compaction's K-th and (K + 1)-th pairs had equal scores: the bound lies inside a run of ties
    status, ids, scores   the list the survivors give: 1 for an empty row; 2 when a live entry's score is not finite (the statistics
                     see every live entry, appended or not), ids / scores then empty; else the min(K, count) best, ordered"""
    ids = np.asarray(ids_row, np.int64)
    E = ids.shape[0]
    assert (np.diff(ids) >= 0).all(), "the plan stage hands the kernel sorted rows"
    live = np.ones(E, bool)
    live[1:] = ids[1:] != ids[:-1]
    longrow = E > CAP
    buf_s, buf_i = np.zeros(0, scores_row.dtype), np.zeros(0, np.int64)
    bound, finite = None, True
    out = dict(longrow=longrow, live=int(live.sum()), compactions=0, appends=0, appends_after=0, idle=[], idle_then_live=[], live_then_idle=[],
               idle_steps=[], bound_in_tie=False)

    def ordered(s, i):
        o = np.lexsort((i, -s))
        return s[o], i[o]
    steps = -(-E // CAND_STEP)
    waves = CAND_STEP // WAVE
    cell_live = np.zeros((waves, steps + 1), bool)                   # (one column past the end: no step, not live)
    cell_in = np.zeros((waves, steps + 1), bool)
    for t in range(steps):
        base = t * CAND_STEP
        if longrow and buf_s.shape[0] + CAND_STEP > CAP:
            buf_s, buf_i = ordered(buf_s, buf_i)
            out["bound_in_tie"] |= bool(buf_s[K - 1] == buf_s[K])
            buf_s, buf_i = buf_s[:K], buf_i[:K]
            bound = (buf_s[K - 1], buf_i[K - 1])
            out["compactions"] += 1
        for w in range(waves):
            cell = live[base + w * WAVE:min(base + (w + 1) * WAVE, E)]
            cell_in[w, t], cell_live[w, t] = cell.shape[0] > 0, cell.any()
        it = ids[base:base + CAND_STEP][live[base:base + CAND_STEP]]
        s = scores_row[it] + scores_row.dtype.type(0)                # (-0 is +0)
        finite &= bool(np.isfinite(s).all())
        if bound is not None:
            keep = (s > bound[0]) | ((s == bound[0]) & (it < bound[1]))
            s, it = s[keep], it[keep]
        buf_s, buf_i = np.concatenate([buf_s, s]), np.concatenate([buf_i, it])
        assert buf_s.shape[0] <= CAP
        out["appends"] += s.shape[0]
        out["appends_after"] += s.shape[0] if out["compactions"] else 0
    for t in range(steps):
        for w in range(waves):
            if cell_in[w, t] and not cell_live[w, t]:
                out["idle"].append((w, t))
                if cell_live[w, t + 1]:
                    out["idle_then_live"].append((w, t))
                if t and cell_live[w, t - 1]:
                    out["live_then_idle"].append((w, t))
        if not cell_live[:, t].any():
            out["idle_steps"].append(t)
    buf_s, buf_i = ordered(buf_s, buf_i)
    out["status"] = 1 if E == 0 else 0 if finite else 2
    out["ids"], out["scores"] = (buf_i[:K], buf_s[:K]) if out["status"] == 0 else (buf_i[:0], buf_s[:0])
    return out


# ---- the cases of tests/test_hip_candidates_structured.py -----------------------------------------------------------------------
# a. order along long rows: the append-everything limit, one entry more, the step behind it and one more, two longer rows; short ones
ORDER_M, ORDER_N = 16, 6000
ORDER_LONG = (2048, 2049, 2304, 2305, 4999, 6000)
ORDER_COUNTS = ORDER_LONG + tuple(range(300, 1801, 166))[:ORDER_M - len(ORDER_LONG)]
ORDER_CASES = [(kind, dtype, kf) for kind in STRUCTURED for dtype, kf in ((F32, 24), (F64, 12))] + [("ascending", F32, 1), ("ascending", F64, 1)]
ORDER_K = (1, 10, 1024)


@functools.lru_cache(maxsize=None)
def order_case(kind, dtype, kf):
    A, B = structured_factors(kind, ORDER_M, ORDER_N, kf, dtype, 21)
    return dict(A=A, B=B, cand=spread_rows(ORDER_COUNTS, ORDER_N, 11))


# b. duplicates at scale
DUP_N = 3000
DUP_TIMES = (64, 65, 128, 256, 300, 2100)
DUP_BASES = ((40, (0, 1, 39)), (900, (0, 256, 257, 899)))            # distinct ids of the base row; positions: start, 64 j, 64 j + 1, end
DUP_CASES = [(F32, 17), (F32, 130), (F64, 9), (F64, 130)]
DUP_K = (10, 1024)


@functools.lru_cache(maxsize=None)
def duplicate_rows():
    """(rows, names): names[u] says what row u is"""
    rng = np.random.default_rng(31)
    base = {c: rows_of(spread_rows((c,), DUP_N, 32 + c))[0] for c in (40, 900, 2047, 2048)}
    rows, names = [], []
    for times in DUP_TIMES:
        for c, ats in DUP_BASES:
            for at in ats:
                rows.append(dup_run(base[c], at, times))
                names.append(("dup_run", c, at, times))
    rows += [np.full(5000, 1234, np.int32), few_distinct(DUP_N, 3000, 500, rng), dup_run(base[2047], 1000, 2), dup_run(base[2048], 1000, 2)]
    names += [("one_id",), ("few_distinct",), ("2048 entries, 2047 distinct",), ("2049 entries, 2048 distinct",)]
    short = [np.sort(rng.choice(np.arange(400 * u, 400 * u + 600), 9, replace=False)) for u in range(4)]
    rows += chained(short) + [np.zeros(0, np.int32)]
    names += [("chained", u) for u in range(4)] + [("empty",)]
    return [np.asarray(r, np.int32) for r in rows], names


DUP_M = len(DUP_TIMES) * sum(len(ats) for _, ats in DUP_BASES) + 9


@functools.lru_cache(maxsize=None)
def duplicate_case(dtype, kf):
    A, B = structured_factors("iid", DUP_M, DUP_N, kf, dtype, 22)
    rows, names = duplicate_rows()
    assert len(rows) == DUP_M
    return dict(A=A, B=B, cand=csr_of(rows), names=names)


# c. non-finite scores in long rows
NF_M, NF_N, NF_ENTRIES = 16, 6000, 5000
NF_CASES = [(order, dtype) for order in ("ascending", "descending") for dtype in (F32, F64)]
NF_K = (10, 1024)
NF_KF = {F32: 24, F64: 12}
NF_UNLISTED = 2000                                                   # a NaN item row nobody lists
NF_SECOND_COMPACTION = 15 * CAND_STEP                                # ascending: compactions in front of steps 8 and 15 (K = 10) / 8 and 12 (K = 1024)


@functools.lru_cache(maxsize=None)
def nonfinite_case(order, dtype):
    """one defect per designed user (`hit`: user -> what); every other user lists none of the damaged items"""
    kf, n = NF_KF[dtype], NF_N
    A, B = (x.copy() for x in structured_factors(order, NF_M, n, kf, dtype, 23))
    huge = {F32: 3e38, F64: 1.7e308}[dtype]
    over = int(np.argmax(A[:, 0]))                                   # A[:, 0] = 1 + |z|: the largest one overflows huge * A[u, 0]
    free = [u for u in range(NF_M) if u != over]
    if order == "ascending":
        items = {free[1]: ("NaN item row in the first step", 3), free[2]: ("NaN item row behind the second compaction", 5600),
                 free[3]: ("NaN item row at the last entry", n - 1), free[4]: ("+Inf in a factor of the last item of the row", n - 2),
                 over: ("finite factors whose product overflows", 3000)}
        B[3], B[5600], B[n - 1], B[n - 2, 0], B[3000, 0] = np.nan, np.nan, np.nan, np.inf, huge
        A[free[5], kf // 2] = np.nan
        hit = {u: what for u, (what, _) in items.items()}
        hit[free[5]] = "NaN in the user's own factors"
    else:
        items = {free[1]: ("-Inf in a factor of the last item of the row", n - 1)}
        B[n - 1, 0] = -np.inf
        hit = {free[1]: items[free[1]][0]}
    B[NF_UNLISTED] = np.nan
    damaged = np.array(sorted({i for _, i in items.values()} | {NF_UNLISTED}))
    rng = np.random.default_rng(24)
    sound = np.setdiff1d(np.arange(n), damaged)
    rows = []
    for u in range(NF_M):
        own = [items[u][1]] if u in items else []
        rows.append(np.sort(np.concatenate([rng.choice(sound, NF_ENTRIES - len(own), replace=False), own])).astype(np.int32))
    return dict(A=A, B=B, cand=csr_of(rows), hit=hit, items={u: i for u, (_, i) in items.items()}, overflow=(over, 3000) if order == "ascending" else None)


# d. factor counts x several steps x layouts
COUNTS_M, COUNTS_N, COUNTS_K = 12, 3000, 10
COUNTS_ROWS = (257, 600, 2305, 0, 1, 5, 63, 64, 65, 255, 256, 130)
COUNTS_CASES = [(F32, kf) for kf in (1, 3, 15, 16, 17, 31, 33, 64, 130)] + [(F64, kf) for kf in (1, 7, 8, 9, 17, 130)]


@functools.lru_cache(maxsize=None)
def counts_case(dtype, kf):
    A, B = structured_factors("iid", COUNTS_M, COUNTS_N, kf, dtype, 25)
    return dict(A=A, B=B, cand=spread_rows(COUNTS_ROWS, COUNTS_N, 26))


# e. batch and shard edges: three batches of 1,024 users, three shards of 700
EDGE_M, EDGE_N, EDGE_KF, EDGE_K = 2100, 3000, 8, 10
EDGE_USERS = (1023, 1024, 2047, 2048, 699, 1399, 2099)
EDGE_ROWS = ("long", "dup_run", "few_distinct", "empty")


@functools.lru_cache(maxsize=None)
def edge_case():
    A, B = structured_factors("ascending", EDGE_M, EDGE_N, EDGE_KF, F32, 27)
    rng = np.random.default_rng(28)
    rows = rows_of(spread_rows(tuple(rng.integers(0, 9, EDGE_M)), EDGE_N, 29))
    special = {"long": rows_of(spread_rows((2305,), EDGE_N, 30))[0], "dup_run": dup_run(rows_of(spread_rows((900,), EDGE_N, 33))[0], 257, 300),
               "few_distinct": few_distinct(EDGE_N, 3000, 500, rng), "empty": np.zeros(0, np.int32)}
    kinds = {u: EDGE_ROWS[j % len(EDGE_ROWS)] for j, u in enumerate(EDGE_USERS)}
    for u, kind in kinds.items():
        rows[u] = special[kind]
    return dict(A=A, B=B, cand=csr_of(rows), kinds=kinds)


FAMILIES = {"order": order_case, "duplicates": duplicate_case, "nonfinite": nonfinite_case, "counts": counts_case, "edges": edge_case}


@functools.lru_cache(maxsize=None)
def scores_of(family, *args):
    """the oracle's scores of a case's factors (the k-ordered fma chain, the bits the device must write); computed once, read-only"""
    from oracle.oracle import Oracle
    case = FAMILIES[family](*args)
    S = Oracle().scores(case["A"], case["B"], dtype=case["A"].dtype.type)
    S.flags.writeable = False
    return S


@functools.lru_cache(maxsize=None)
def want_of(family, K, *args):
    """the reference lists of a case: test_hip_recommend's checker on the complement of the candidate rows; computed once, read-only"""
    from test_hip_recommend import expected_lists
    case = FAMILIES[family](*args)
    want = expected_lists(scores_of(family, *args), complement_of(case["cand"], case["B"].shape[0]), K)
    for w in want:
        w.flags.writeable = False
    return want
