"""Synthetic MovieLens-/MSD-shaped inputs for tests and bench.py.

Factors ``A, B ~ N(0,1)/sqrt(k)`` (scores ~ N(0,1), tie-free with overwhelming probability);
per-user interaction counts ``clip(round(lognormal(mu, 1)), 2, n/4)`` with the requested mean;
items uniform without replacement, sorted; ``max(1, round(0.3*c))`` of them held out as the test
row (the reference's default ``items_test_fraction``, recometrics/__init__.py:635), the rest is
the train row; test values uniform in {1..20}.
"""
import numpy as np

CONFIGS = {
    # name: (m, n, k, dtype, K, mean interactions, seed)
    "C1": (1_000, 5_000, 64, np.float32, 10, 50, 101),
    "C2": (138_493, 26_744, 64, np.float32, 10, 144, 102),
    "C3": (1_000_000, 380_000, 128, np.float32, 20, 48, 103),
    "C4": (100_000, 10_000_000, 128, np.float32, 100, 10, 104),
    "C5": (200_000, 500_000, 256, np.float64, 50, 50, 105),
    "NS": (32_768, 1_000_000, 128, np.float32, 10, 100, 100),
    # the only realistic workload the reference documents (examples/recometrics_example.ipynb cells 3, 5, 9, 11; BASELINE.md
    # section 1): LastFM-360K -- 10,000 test users x 160,112 items, 50 factors, k = 5, all metrics, API defaults (noise on)
    "TUT": (10_000, 160_112, 50, np.float32, 5, 50, 108),
    # probes (not BASELINE configs): fp64 with resident user factors / small K
    "P64a": (8_192, 500_000, 128, np.float64, 10, 50, 106),
    "P64b": (8_192, 500_000, 256, np.float64, 10, 50, 107),
}


def make_factors(m, n, k, dtype=np.float32, seed=0):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((m, k), dtype=np.float32) / np.sqrt(k)).astype(dtype)
    B = (rng.standard_normal((n, k), dtype=np.float32) / np.sqrt(k)).astype(dtype)
    return A, B


def make_interactions(m, n, mean_c, dtype=np.float32, seed=0, test_fraction=0.3):
    """Returns (train_indptr, train_indices, test_indptr, test_indices, test_values)."""
    rng = np.random.default_rng(seed + 7919)
    mu = np.log(max(mean_c, 1.0)) - 0.5
    c = np.clip(np.rint(rng.lognormal(mu, 1.0, size=m)), 2, max(2, n // 4)).astype(np.int64)
    # draw with a little slack, dedupe per user
    tr_p = np.zeros(m + 1, dtype=np.int64)
    te_p = np.zeros(m + 1, dtype=np.int64)
    tr_chunks, te_chunks = [], []
    for u in range(m):
        cu = int(c[u])
        items = np.unique(rng.integers(0, n, size=cu + (cu >> 3) + 2))
        if items.shape[0] > cu:
            items = np.sort(rng.permutation(items)[:cu])
        cu = items.shape[0]
        nte = min(max(1, int(round(test_fraction * cu))), cu)
        pick = np.zeros(cu, dtype=bool)
        pick[rng.permutation(cu)[:nte]] = True
        te_chunks.append(items[pick])
        tr_chunks.append(items[~pick])
        te_p[u + 1] = te_p[u] + nte
        tr_p[u + 1] = tr_p[u] + (cu - nte)
    tr_i = np.concatenate(tr_chunks).astype(np.int32) if tr_chunks else np.zeros(0, np.int32)
    te_i = np.concatenate(te_chunks).astype(np.int32) if te_chunks else np.zeros(0, np.int32)
    te_v = rng.integers(1, 21, size=te_i.shape[0]).astype(dtype)
    return tr_p.astype(np.int32), tr_i, te_p.astype(np.int32), te_i, te_v


def make_interactions_fast(m, n, mean_c, dtype=np.float32, seed=0, test_fraction=0.3):
    """The same kind of data as make_interactions (lognormal row lengths, uniform items, ~30 % of a row held out, at least one test
    item per user), drawn in whole-array operations: seconds instead of minutes for a million users.  NOT the same draws -- the
    workloads bench.py times keep make_interactions; this one feeds the tests that run a BASELINE config at its full user count."""
    rng = np.random.default_rng(seed + 104729)
    mu = np.log(max(mean_c, 1.0)) - 0.5
    c = np.clip(np.rint(rng.lognormal(mu, 1.0, size=m)), 2, max(2, n // 4)).astype(np.int64)
    users = np.repeat(np.arange(m, dtype=np.int64), c)
    key = np.unique(users * np.int64(n) + rng.integers(0, n, size=users.shape[0], dtype=np.int64))      # sorted by (user, item), duplicates dropped
    users, items = key // n, (key % n).astype(np.int32)
    del key
    start = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(users, minlength=m), out=start[1:])
    held = rng.random(users.shape[0]) < test_fraction
    none = np.bincount(users[held], minlength=m) == 0                    # users without a test item: their first entry becomes one
    held[start[:-1][none & (start[1:] > start[:-1])]] = True
    all_held = (np.bincount(users[~held], minlength=m) == 0) & (start[1:] - start[:-1] > 1)      # ... and nobody loses the whole row
    held[start[:-1][all_held]] = False
    te_p = np.zeros(m + 1, np.int64); tr_p = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(users[held], minlength=m), out=te_p[1:])
    np.cumsum(np.bincount(users[~held], minlength=m), out=tr_p[1:])
    te_i, tr_i = items[held], items[~held]
    te_v = rng.integers(1, 21, size=te_i.shape[0]).astype(dtype)
    return tr_p.astype(np.int32), tr_i, te_p.astype(np.int32), te_i, te_v


def make_problem(m, n, k, dtype=np.float32, mean_c=50, seed=0):
    A, B = make_factors(m, n, k, dtype, seed)
    trp, tri, tep, tei, tev = make_interactions(m, n, mean_c, dtype, seed)
    return {"A": A, "B": B, "train": (trp, tri), "test": (tep, tei, tev)}


# ---- ordered and structured scores ---------------------------------------------------------------------------------------------
# make_factors gives every user scores that are i.i.d. IN ITEM ORDER: a streaming top-K then sees a new best only ~ K ln(n / K)
# times in n items.  Catalogues sorted by popularity or release date are not like that.  The kinds below put the order, the ties
# and the outliers into the FACTORS, so that the same arrays go through every entry point; none of them touches the draws above.
STRUCTURED_KINDS = ("ascending", "descending", "trend", "planted", "outliers", "runs")


def _ramp(n, dtype, rng, span):
    """n distinct ascending values in [-span, span]: an even grid, every point moved by less than a quarter of a step"""
    step = 2.0 * span / max(n - 1, 1)
    r = (np.linspace(-span, span, n) + rng.uniform(-0.25, 0.25, n) * step).astype(dtype)
    if n > 1 and not (np.diff(r.astype(np.float64)) > 8 * np.finfo(dtype).eps * span).all():
        raise ValueError("%d distinct values do not fit [-%g, %g] in %s" % (n, span, span, np.dtype(dtype).name))
    return r


def _ordered_factors(m, n, k, dtype, rng, span, descending=False, jitter=0.0, dup=0.0):
    """score(u, i) = a_u * ramp_i (+ personal noise): a_u = 1 + |z| > 0, so every user's scores follow the ramp.  The columns
    behind the first hold zeros in B (jitter == 0): the k-ordered fma chain adds exact zeros to fl(a_u * ramp_i), and the product
    of a positive number with distinct values a few ulp apart stays strictly monotone."""
    ramp = _ramp(n, dtype, rng, span)
    if descending:
        ramp = ramp[::-1]
    A = np.ones((m, k), dtype)
    B = np.zeros((n, k), dtype)
    B[:, 0] = ramp
    if k > 1:
        A[:, 0] = (1.0 + np.abs(rng.standard_normal(m))).astype(dtype)
        A[:, 1:] = (rng.standard_normal((m, k - 1)) / np.sqrt(k)).astype(dtype)
        if jitter:
            B[:, 1:] = (rng.standard_normal((n, k - 1)) * jitter).astype(dtype)
    if dup:                                                   # rows equal to their predecessor's: runs of exactly tied scores
        same = rng.random(n) < dup
        same[0] = False
        src = np.maximum.accumulate(np.where(same, 0, np.arange(n)))
        B = B[src]
    return A, np.ascontiguousarray(B)


def _planted(m, n, k, dtype, mean_c, rng, beta, test_fraction):
    """low-rank taste (up to 8 factors) + one popularity column with a Zipf tail + small noise in the remaining columns; a user's
    items are drawn without replacement with probability ~ exp(beta * score) (Gumbel top-c on the float64 scores), then split into
    train and test at random: the positives sit near the top of the ranking."""
    r = max(0, min(8, k - 1))
    A = np.zeros((m, k), dtype)
    B = np.zeros((n, k), dtype)
    A[:, :r] = rng.standard_normal((m, r)).astype(dtype)
    B[:, :r] = (rng.standard_normal((n, r)) / np.sqrt(max(r, 1))).astype(dtype)
    A[:, r] = 1
    B[:, r] = (3.0 / np.sqrt(rng.permutation(n) + 1.0)).astype(dtype)            # a few blockbusters, a long flat tail
    if k > r + 1:
        A[:, r + 1:] = (rng.standard_normal((m, k - r - 1)) / np.sqrt(k)).astype(dtype)
        B[:, r + 1:] = (rng.standard_normal((n, k - r - 1)) * 0.05).astype(dtype)
    mu = np.log(max(mean_c, 1.0)) - 0.5
    c = np.clip(np.rint(rng.lognormal(mu, 1.0, size=m)), 2, max(2, n // 4)).astype(np.int64)
    B64 = B.astype(np.float64)
    tr_rows, te_rows = [], []
    for u in range(m):
        key = beta * (B64 @ A[u].astype(np.float64)) + rng.gumbel(size=n)
        items = np.argpartition(-key, int(c[u]) - 1)[:int(c[u])]
        nte = min(max(1, int(round(test_fraction * items.shape[0]))), items.shape[0])
        pick = np.zeros(items.shape[0], bool)
        pick[rng.permutation(items.shape[0])[:nte]] = True
        te_rows.append(np.sort(items[pick]))
        tr_rows.append(np.sort(items[~pick]))
    def csr(rows):
        p = np.zeros(m + 1, np.int64)
        np.cumsum([x.shape[0] for x in rows], out=p[1:])
        return p.astype(np.int32), np.concatenate(rows).astype(np.int32)
    trp, tri = csr(tr_rows)
    tep, tei = csr(te_rows)
    tev = rng.integers(1, 21, size=tei.shape[0]).astype(dtype)
    return A, B, (trp, tri), (tep, tei, tev)


def _outliers(m, n, k, dtype, rng, variant):
    """"spikes": every score within +-1e-3 except a handful of items per user group at +-1e3 ... 1e6 (up to four groups of users,
    each with spike items of its own); "clusters": two clusters of scores at +-a_u, each 1e-3 wide, nothing in between."""
    if k < 2:
        raise ValueError("outliers needs at least 2 factors")
    g = 1 if variant == "clusters" else min(4, k - 1)
    A = np.zeros((m, k), dtype)
    B = np.zeros((n, k), dtype)
    A[:, g:] = rng.uniform(-1, 1, (m, k - g)).astype(dtype)
    B[:, g:] = (rng.uniform(-1, 1, (n, k - g)) * (1e-3 / (k - g))).astype(dtype)      # |bulk score| <= 1e-3
    a = (1.0 + np.abs(rng.standard_normal(m))).astype(dtype)
    if variant == "clusters":
        A[:, 0] = a
        B[:, 0] = rng.choice(np.array([-1, 1], dtype), n)
    elif variant == "spikes":
        A[np.arange(m), np.arange(m) % g] = a * rng.choice(np.array([-1, 1], dtype), m)
        for c in range(g):
            items = rng.permutation(n)[:min(n, 12)]
            B[items, c] = (10.0 ** rng.uniform(3, 6, items.shape[0]) * rng.choice([-1.0, 1.0], items.shape[0])).astype(dtype)
    else:
        raise ValueError("outliers variant %r" % (variant,))
    return A, B


def make_structured(kind, m, n, k, dtype=np.float32, mean_c=50, seed=0, jitter=0.3, dup=0.2, beta=2.2, span=4.0,
                    variant="spikes", test_fraction=0.3, interactions=make_interactions):
    """The same dict as make_problem, with scores that are ordered or structured along the item axis:

    ascending / descending  strictly monotone in the item id for every user, tie-free (k == 1: A = 1, B = the ramp -- the
                            folded item_biases call; k > 1: A[:, 0] = 1 + |z|, B[:, 0] = the ramp, B[:, 1:] = 0)
    trend                   the ascending ramp under personal noise, B[:, 1:] ~ N(0, jitter)
    planted                 taste + Zipf popularity, interactions drawn ~ exp(beta * score): positives near the top
    outliers                variant "spikes" or "clusters" (see _outliers)
    runs                    ascending with a fraction `dup` of the item rows equal to their predecessor's: exact ties in order

    Interactions come from `interactions` (make_interactions, or make_interactions_fast for a full user count) except for planted."""
    rng = np.random.default_rng([seed, 15485863])
    if kind == "planted":
        A, B, train, test = _planted(m, n, k, dtype, mean_c, rng, beta, test_fraction)
        return {"A": A, "B": B, "train": train, "test": test}
    if kind in ("ascending", "descending"):
        A, B = _ordered_factors(m, n, k, dtype, rng, span, descending=kind == "descending")
    elif kind == "trend":
        A, B = _ordered_factors(m, n, k, dtype, rng, span, jitter=jitter)
    elif kind == "runs":
        A, B = _ordered_factors(m, n, k, dtype, rng, span, dup=dup)
    elif kind == "outliers":
        A, B = _outliers(m, n, k, dtype, rng, variant)
    else:
        raise ValueError("unknown kind %r (one of %s)" % (kind, ", ".join(STRUCTURED_KINDS)))
    trp, tri, tep, tei, tev = interactions(m, n, mean_c, dtype, seed, test_fraction)
    return {"A": A, "B": B, "train": (trp, tri), "test": (tep, tei, tev)}


def permute_items(pr, perm):
    """The same problem with its items relabelled: old item i becomes item perm[i] (rows of B moved, CSR indices of train and test
    mapped, every row sorted again with its test values).  A score belongs to a (user, item) pair, so nothing changes but the order
    in which a sweep over the item axis meets the scores.  permute_items(permute_items(pr, perm), np.argsort(perm)) is pr."""
    perm = np.asarray(perm, dtype=np.int64)
    n = pr["B"].shape[0]
    if perm.shape != (n,) or not (np.sort(perm) == np.arange(n)).all():
        raise ValueError("perm must be a permutation of the %d items" % n)
    B = np.empty_like(pr["B"])
    B[perm] = pr["B"]

    def relabel(indptr, indices, values=None):
        users = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
        new = perm[indices]
        order = np.argsort(users * n + new, kind="stable")
        out = (indptr.copy(), new[order].astype(indices.dtype))
        return out if values is None else out + (values[order],)
    test = pr["test"]
    return {"A": pr["A"], "B": B, "train": relabel(*pr["train"][:2]),
            "test": relabel(test[0], test[1], test[2] if len(test) > 2 else None)}
