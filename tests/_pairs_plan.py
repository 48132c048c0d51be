"""A pairwise plan of small metric calls over every option of a call, written as data.

Pure Python, no random numbers: nothing here is imported from the product, and the list comes out the same on every run and every
Python.  tests/test_pairs_plan_cpu.py checks the plan against the table of dimensions and the oracle without a GPU;
tests/test_hip_pairs.py walks it on one.

A case is one level of every dimension.  The plan is a list of cases in which EVERY ALLOWED PAIR of levels of two different
dimensions occurs at least once: the suite's other files vary one or two options and hold the rest at their defaults, so two
options meet there only where somebody thought of the combination.  The problems the cases run on are built by tests/_pairs.py."""
import collections
import itertools

# ---- the dimensions and their levels ------------------------------------------------------------------------------------------------
DIMENSIONS = collections.OrderedDict([
    ("entry", ("factors", "scores")),            # calc_metrics from (A, B); calc_metrics_scores with S = oracle.scores(A, B)
    ("dtype", ("f32", "f64")),
    ("K", (1, 10, 33, 100, 300)),                # fp32: lists in LDS (1, 10), lane buffers + k_collect_topk (33, 100, 300); fp64: lane buffers.
                                                 # (At 300 the lane buffers still fit 200 users: no factor case stores score rows for
                                                 # k_select_topk.  The score-matrix entry selects from stored rows at every k_metrics.)
    ("request", ("all", "default", "topk8", "p+roc", "ndcg", "pr", "hit+rr")),
    ("cumulative", ("single", "cumulative")),
    ("noise", ("off", "on")),                    # on: seed = 2 ** 33 + 5
    ("eligibility", ("defaults", "strict")),     # strict: cold=False, min_pos_test=3, min_items_pool=50
    ("structure", ("iid", "runs", "ascending", "zero_rows")),
    ("overlap", ("none", "third")),              # third: every third user's train row gains 30 % of its test items
    ("batches", ("one", "64")),                  # RM_BATCH_USERS=64: the score-matrix entry only (EXCLUDED)
    ("devices", ("one", "three")),               # rm_set_devices [0] / [0, 0, 0]
    ("splits", ("default", "3")),                # RM_DEBUG_SPLITS=3
])
NAMES = tuple(DIMENSIONS)

REQUESTS = {"all": ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr", "roc", "pr"), "default": ("p", "ap", "ndcg"),
            "topk8": ("p", "tp", "r", "ap", "tap", "ndcg", "hit", "rr"), "p+roc": ("p", "roc"), "ndcg": ("ndcg",), "pr": ("pr",),
            "hit+rr": ("hit", "rr")}
NOISE_SEED = 2 ** 33 + 5
STRICT = dict(cold=False, min_pos_test=3, min_items_pool=50)
ENV = {("batches", "64"): ("RM_BATCH_USERS", "64"), ("splits", "3"): ("RM_DEBUG_SPLITS", "3")}
DEVICES = {"one": [0], "three": [0, 0, 0]}

# Pairs of levels that no call of this family can have: ((dimension, level), (dimension, level), why).  Nothing else is excluded.
EXCLUDED = (
    (("entry", "scores"), ("noise", "on"), "the score-matrix entry has no tie noise"),
    (("entry", "scores"), ("splits", "3"), "the score-matrix entry has no sweep"),
    (("entry", "factors"), ("batches", "64"), "from factors a batch holds whole 1,024s of users whatever RM_BATCH_USERS says (csrc/rm_lib.hip "
                                              "batch_users_max): the family's 200 users are one batch, the call would be batches = one's"),
)

# What EXCLUDED implies: pairs that are not excluded themselves and that no case can hold, because either level leaves the entry no
# choice and the two choices differ.  ((dimension, level), (dimension, level), the file that has them meet on the GPU, or None).
# tests/test_pairs_plan_cpu.py recomputes this list from EXCLUDED.  The plan does NOT cover them.
UNREACHABLE = (
    (("noise", "on"), ("batches", "64"), "tests/test_hip_entry_fields.py, tests/test_hip_multi.py, tests/test_hip_requests.py: 2,500 users and more"),
    (("batches", "64"), ("splits", "3"), None),
)

# A constraint on TRIPLES, not an exclusion of pairs -- cases that would check nothing, as triples of (dimension, level): at
# k_metrics = 1 the best score IS the K-th, so without ROC-AUC and without the noise the partial validity rule
# (oracle/recometrics_oracle.cpp: hi == lo) holds every user invalid, on any input.
# No pair is lost to them: (K = 1, request) is met with the noise on, (K = 1, noise off) under a request with ROC-AUC.
EMPTY = tuple((("K", 1), ("noise", "off"), ("request", req)) for req in DIMENSIONS["request"] if "roc" not in REQUESTS[req])

# Triples the plan must hold, beyond the pairs: the generator begins with them.  A request without ROC-AUC differs from the all-ten
# call only where the partial validity rule decides -- noise off, a user's best K scores exactly tied, which `runs` plants for
# every third user.  All pairs covered, the two requests could still meet `runs` only with the noise on, and decide nothing.
REQUIRED = tuple((("request", req), ("noise", "off"), ("structure", "runs")) for req in ("pr", "hit+rr"))

Case = collections.namedtuple("Case", NAMES)


def _excluded_pairs():
    return {frozenset((a, b)) for a, b, _ in EXCLUDED + UNREACHABLE}


def allowed_pairs():
    """every pair of (dimension, level) of two different dimensions, less EXCLUDED and what it implies (UNREACHABLE)"""
    out = []
    for d1, d2 in itertools.combinations(NAMES, 2):
        for l1 in DIMENSIONS[d1]:
            for l2 in DIMENSIONS[d2]:
                if frozenset(((d1, l1), (d2, l2))) not in _excluded_pairs():
                    out.append(((d1, l1), (d2, l2)))
    return out


def pairs_of(case):
    levels = [(d, getattr(case, d)) for d in NAMES]
    return [(a, b) for a, b in itertools.combinations(levels, 2)]


def is_valid(levels):
    """`levels`: {dimension: level}, whole or partial -- no excluded pair, no empty triple among what is set"""
    have = set(levels.items())
    if any(a in have and b in have for a, b, _ in EXCLUDED):
        return False
    return not any(all(t in have for t in triple) for triple in EMPTY)


_UNDER_A_RULE = {a[0] for a, b, _ in EXCLUDED} | {b[0] for a, b, _ in EXCLUDED} | {d for triple in EMPTY for d, _ in triple}
_CONSTRAINED = tuple(d for d in NAMES if d in _UNDER_A_RULE)


def can_be_completed(levels):
    """a partial case that some choice of the dimensions under a rule still completes"""
    free = [d for d in _CONSTRAINED if d not in levels]
    for choice in itertools.product(*[DIMENSIONS[d] for d in free]):
        trial = dict(levels)
        trial.update(zip(free, choice))
        if is_valid(trial):
            return True
    return False


def _generate():
    """Deterministic greedy construction: a case starts from the first pair not yet met and takes, dimension by dimension in the
    table's order, the level that meets the most pairs not yet met with the levels already set (the first such level on a draw;
    among levels that meet nothing new, the one the plan has used least).  The first cases start from REQUIRED's triples instead.
    Ends when every allowed pair is met."""
    todo = collections.OrderedDict((frozenset(p), p) for p in allowed_pairs())
    used = collections.Counter()
    cases = []
    required = list(REQUIRED)
    while todo or required:
        first = required.pop(0) if required else next(iter(todo.values()))
        levels = dict(first)
        assert can_be_completed(levels), first
        for d in NAMES:
            if d in levels:
                continue
            best, best_key = None, None
            for i, lv in enumerate(DIMENSIONS[d]):
                trial = dict(levels)
                trial[d] = lv
                if not can_be_completed(trial):
                    continue
                gain = sum(1 for other in levels.items() if frozenset(((d, lv), other)) in todo)
                key = (-gain, used[(d, lv)], i)
                if best_key is None or key < best_key:
                    best, best_key = lv, key
            assert best is not None, (levels, d)
            levels[d] = best
        case = Case(**levels)
        assert is_valid(dict(zip(NAMES, case))), case
        for p in pairs_of(case):
            todo.pop(frozenset(p), None)
        for d in NAMES:
            used[(d, getattr(case, d))] += 1
        cases.append(case)
    return cases


CASES = _generate()


def case_id(case):
    """the levels, spelled: factors-f32-K10-all-single-noise_off-elig_defaults-iid-overlap_none-batches_one-dev_one-splits_default"""
    return "-".join([case.entry, case.dtype, "K%d" % case.K, case.request, case.cumulative, "noise_" + case.noise, "elig_" + case.eligibility,
                     case.structure, "overlap_" + case.overlap, "batches_" + case.batches, "dev_" + case.devices, "splits_" + case.splits])


def call_kw(case):
    """the keywords of oracle.calc (and of the device call) that the case sets"""
    kw = dict(metrics=REQUESTS[case.request], cumulative=case.cumulative == "cumulative", noise=case.noise == "on")
    if kw["noise"]:
        kw["seed"] = NOISE_SEED
    if case.eligibility == "strict":
        kw.update(STRICT)
    return kw


def env_of(case):
    return dict(ENV[(d, getattr(case, d))] for d in ("batches", "splits") if (d, getattr(case, d)) in ENV)


def shard_ranges(m, shards):
    """the user ranges of a call on `shards` devices (csrc/rm_lib.hip: m g / G)"""
    return [(m * g // shards, m * (g + 1) // shards) for g in range(shards)]


def batch_cuts(m, batch):
    """the batch boundaries of a range of m users under RM_BATCH_USERS=batch, which the score-matrix entry takes as it is (csrc/rm_lib.hip
    batch_cuts, forced: equal batches and what is left); None: the one batch of a small range"""
    return list(range(0, m, batch or m)) + [m]


def cuts_of(case, m):
    """per user range of the case's call, in the device list's order: the batch boundaries inside the range"""
    batch = int(ENV[("batches", "64")][1]) if case.batches == "64" else None
    return [batch_cuts(u1 - u0, batch) for u0, u1 in shard_ranges(m, len(DEVICES[case.devices]))]
