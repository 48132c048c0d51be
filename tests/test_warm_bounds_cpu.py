"""CPU-only: tests/_warm_bounds.py, the NumPy restatement of k_hint_bounds' rejection rules that the GPU test uses as its expectation,
on problems small enough to check by hand, and on the GPU test's split."""
import numpy as np

import _warm_bounds as wb


def _csr(rows):
    p = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=p[1:])
    return p, np.array([i for r in rows for i in r], np.int32)


N, K = 12, 3
TRAIN = [[0, 1], [2, 3, 4], [], [0, 1, 2, 3, 4, 5, 6, 7, 8], [5], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]]
TEST = [[5, 6], [0], [7], [9, 10], [], [10, 11]]
#        ok     ok   cold  ok      no test row   12 - 10 = 2 candidates < K: not evaluated


def test_who_is_evaluated_for_ranks_in_one_slot():
    trp, _ = _csr(TRAIN)
    tep, _ = _csr(TEST)
    assert wb.evaluated_for_ranks(N, K, trp, tep).tolist() == [True, True, True, True, False, False]
    assert wb.evaluated_for_ranks(N, K, trp, tep, cold=False).tolist() == [True, True, False, True, False, False]
    # a user whose train and test rows cover every item has an NDCG and nothing else
    trp2, _ = _csr([[0, 1, 2, 3, 4, 5, 6, 7]])
    tep2, _ = _csr([[8, 9, 10, 11]])
    assert wb.evaluated_for_ranks(N, K, trp2, tep2).tolist() == [False]
    # more than 63 test items: one slot when the long rows are streamed, several otherwise
    trp3, _ = _csr([[0], [0]])
    tep3, _ = _csr([list(range(1, 65)), list(range(1, 64))])
    assert wb.evaluated_for_ranks(200, K, trp3, tep3).tolist() == [True, True]
    assert wb.evaluated_for_ranks(200, K, trp3, tep3, streamed=False).tolist() == [False, True]


def test_each_rejection_rule():
    trp, tri = _csr(TRAIN)
    tep, _ = _csr(TEST)
    good = np.array([[5, 6, 7], [0, 1, 5], [7, 0, 1], [9, 10, 11], [0, 1, 2], [10, 11, 0]], np.int32)
    assert wb.hintable(good, N, trp, tri, tep).tolist() == [True, True, True, True, False, False]
    for u, bad in ((0, [5, 5, 7]), (0, [5, 6, 1]), (1, [0, 1, -1]), (1, [0, 1, N]), (2, [7, 0, 7]), (3, [9, 10, 8]), (3, [-1, -1, -1])):
        ids = good.copy()
        ids[u] = bad
        want = [True, True, True, True, False, False]
        want[u] = False
        assert wb.hintable(ids, N, trp, tri, tep).tolist() == want, (u, bad)
    # test items are candidates: a user's own test items are acceptable advice
    ids = good.copy()
    ids[0] = [6, 5, 11]
    assert wb.hintable(ids, N, trp, tri, tep)[0]


def test_lists_are_ordered_by_score_then_item_and_padded():
    trp, tri = _csr(TRAIN)
    S = np.tile(np.arange(N, dtype=np.float32), (6, 1))
    S[0, 11] = S[0, 10]                                      # an exact tie: the smaller item first
    L = wb.lists_of(S, trp, tri, K)
    assert L[0].tolist() == [10, 11, 9] and L[1].tolist() == [11, 10, 9] and L[3].tolist() == [11, 10, 9]
    assert L[5].tolist() == [11, 10, -1]


def test_the_poisons_on_the_gpu_tests_split():
    """every kind finds users on the split of tests/_warm_bounds_child.py (rebuilt here without torch), the unacceptable kinds take
    exactly their users out and the test items take nobody out"""
    from recometrics_amd.synth import make_factors, make_interactions
    m, n, k = 300, 700, 10
    trp, tri, tep, tei, _ = make_interactions(m, n, 120, np.float32, seed=5, test_fraction=0.5)
    A, B = make_factors(m, n, 16, np.float32, seed=100)
    lists = wb.lists_of(A.astype(np.float64) @ B.astype(np.float64).T, trp, tri, k)
    base = wb.hintable(lists, n, trp, tri, tep)
    assert base.sum() == wb.evaluated_for_ranks(n, k, trp, tep).sum() > 250
    for kind in wb.POISONS:
        ids, users = wb.poisoned(kind, lists, n, trp, tri, tep, tei)
        assert users.shape[0] >= 20, kind
        after = wb.hintable(ids, n, trp, tri, tep)
        untouched = np.setdiff1d(np.arange(m), users)
        assert (ids[untouched] == lists[untouched]).all() and (after[untouched] == base[untouched]).all(), kind
        assert after[users].all() if kind == "test_items" else not after[users].any(), kind
