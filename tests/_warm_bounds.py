"""The warm top-K bounds (k_hint_bounds) restated in NumPy: which users may get a bound from a given array of
advised item ids, the lists a call leaves behind, and the poisoned advice of the GPU tests.  Nothing here is imported from the product;
tests/test_warm_bounds_cpu.py checks this module without a GPU, tests/_warm_bounds_child.py uses it as the expectation."""
import numpy as np

POS_CHUNK = 63          # test items per sweep slot (rm_device.hpp)


def evaluated_for_ranks(n, K, train_p, test_p, cold=True, min_items_pool=2, min_pos_test=1, streamed=True):
    """[m] bool: the users a call with all ten metrics evaluates, with ROC / PR-AUC, in ONE sweep slot (k_classify restated): a test row,
    at least max(min_items_pool, K, 2) candidates, a train row unless cold-start users count, some item that is neither train nor test
    (else the user only has an NDCG), and a test row of one chunk -- or any length when long rows are streamed."""
    ntr, npos = np.diff(train_p), np.diff(test_p)
    cand = n - ntr
    active = (npos > 0) & (cand >= max(min_items_pool, K, 2)) & (npos >= min(min_pos_test, 1))
    if not cold:
        active &= ntr > 0
    only_ndcg = ntr + npos >= n
    one_slot = np.ones_like(active) if streamed else npos <= POS_CHUNK
    return active & ~only_ndcg & one_slot


def hintable(ids, n, train_p, train_i, test_p, **classify):
    """[m] bool: the users whose K advised ids (`ids` [m, K]) k_hint_bounds accepts -- evaluated for ranks in one slot, at least K
    candidates, every id in [0, n), the K ids pairwise distinct, none a train item of the user.  (Finite scores are the kernel's last
    condition; they depend on the factors, not on the advice.)"""
    ids = np.asarray(ids)
    m, K = ids.shape
    ok = evaluated_for_ranks(n, K, train_p, test_p, **classify) & (n - np.diff(train_p) >= K)
    ok &= ((ids >= 0) & (ids < n)).all(axis=1)
    srt = np.sort(ids, axis=1)
    ok &= (srt[:, 1:] != srt[:, :-1]).all(axis=1)
    for u in np.flatnonzero(ok):
        ok[u] = not np.isin(ids[u], train_i[train_p[u]:train_p[u + 1]]).any()
    return ok


def lists_of(S, train_p, train_i, K):
    """[m, K] int32: every user's K best items outside its train row by (score descending, item ascending), -1 where the user has
    fewer candidates -- what a call leaves as its lists for the users it evaluates (scores without NaN, infinities or signed zeros)"""
    m, n = S.shape
    out = np.full((m, K), -1, np.int32)
    items = np.arange(n)
    for u in range(m):
        cand = np.setdiff1d(items, train_i[train_p[u]:train_p[u + 1]])
        best = cand[np.lexsort((cand, -S[u, cand]))[:K]]
        out[u, :best.shape[0]] = best
    return out


POISONS = ("duplicates", "train_item", "minus_one", "index_n", "other_user", "test_items")


def poisoned(kind, ids, n, train_p, train_i, test_p, test_i, every=3):
    """(ids', users): a copy of `ids` with the advice of some users replaced, and those users.  Every kind but "test_items" makes the
    advice of its users unacceptable; "test_items" hands a user K of its own test items, which are candidates like any other.
    Users are taken from every `every`-th one with acceptable advice, where the kind applies."""
    ids = np.array(ids, np.int32)
    given = ids.copy()
    m, K = ids.shape
    good = np.flatnonzero(hintable(ids, n, train_p, train_i, test_p))[::every]
    users = []
    for u in good:
        tr = train_i[train_p[u]:train_p[u + 1]]
        te = test_i[test_p[u]:test_p[u + 1]]
        if kind == "duplicates":
            if K < 2:
                continue
            ids[u, K - 1] = ids[u, 0]
        elif kind == "train_item":
            if tr.shape[0] == 0:
                continue
            ids[u, u % K] = tr[u % tr.shape[0]]
        elif kind == "minus_one":
            ids[u, u % K] = -1
        elif kind == "index_n":
            ids[u, u % K] = n
        elif kind == "other_user":          # the list of the next user whose list holds a train item of this one
            v = next((v for v in list(range(u + 1, m)) + list(range(u)) if (given[v] >= 0).all() and np.isin(given[v], tr).any()), None)
            if v is None:
                continue
            ids[u] = given[v]
        elif kind == "test_items":
            own = np.setdiff1d(te, tr)
            if own.shape[0] < K:
                continue
            ids[u] = own[::-1][:K]
        else:
            raise ValueError(kind)
        users.append(int(u))
    return ids, np.array(users, np.int64)
