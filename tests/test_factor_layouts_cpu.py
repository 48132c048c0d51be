"""No GPU: the layouts of tests/_layouts.py are what they say, the pair list covers them, and the special-value case of
tests/test_hip_factor_layouts.py is neither empty nor degenerate on the oracle.

place() is what every strided device call of the GPU file stands on: a view that is not the factors, a gap that is not poisoned or a
base that is aligned after all would let those tests pass without having shown anything."""
import functools

import numpy as np
import pytest

import _layouts as lay
from _parity import NT
from _requests import ALL, TOPK8
from _util import bits, same_bits
from test_hip_sweep_rows import DTYPE, M_USERS, NO_TEST_USERS, problem

SHAPES = ((1, 1), (7, 13), (5, 16), (33, 260))
POISONS = {"nan": lay.NAN_POISON, "big": lay.BIG_POISON}


def is_poison(x, poison):
    return np.isnan(x) if np.isnan(poison) else bits(np.ascontiguousarray(x)) == bits(np.full(1, poison, x.dtype))[0]


@pytest.mark.parametrize("poison", sorted(POISONS))
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(lay.LAYOUTS))
def test_place_gives_the_layout_it_names(name, prec, poison):
    dtype, (pad, off), p = DTYPE[prec], lay.LAYOUTS[name][prec], POISONS[poison][prec]
    for m, k in SHAPES:
        X = np.random.default_rng(m * 1000 + k).standard_normal((m, k)).astype(dtype)
        X[0, 0] = -0.0                                                # (bitwise: a copy through arithmetic would lose the sign)
        V, raw, at = lay.place_as(X, name, p)
        assert V.shape == X.shape and V.dtype == X.dtype and raw.ndim == 1 and raw.dtype == X.dtype
        assert (bits(np.ascontiguousarray(V)) == bits(X)).all()
        assert V.strides == ((k + pad) * X.itemsize, X.itemsize)
        assert raw.ctypes.data % 16 == 0 and at == off
        assert V.ctypes.data == raw.ctypes.data + at * X.itemsize and np.shares_memory(V, raw)
        assert (V.ctypes.data - off * X.itemsize) % 16 == 0
        assert V.ctypes.data % 16 == (off * X.itemsize) % 16
        out = lay.outside(V, raw, at)
        assert out.shape[0] == raw.shape[0] - m * k == off + m * pad + lay.TAIL
        assert is_poison(out, p).all()
        # the three kinds of gap, by their places
        assert is_poison(raw[:at], p).all() and is_poison(raw[at + m * (k + pad):], p).all() and raw[at + m * (k + pad):].shape[0] == lay.TAIL
        assert is_poison(raw[at:at + m * (k + pad)].reshape(m, k + pad)[:, k:], p).all()
        C = np.ascontiguousarray(V)
        assert C.flags.c_contiguous and C.shape == X.shape and (bits(C) == bits(X)).all()


def test_the_layouts_are_the_ones_the_kernels_tell_apart():
    """in bytes, at the factor counts the GPU file uses: what `(base | ld * sizeof(T)) & 15` and `ld == k` see"""
    for prec, size in (("f32", 4), ("f64", 8)):
        for k in (16, 13, 260):
            geo = {name: (((k + pad) * size) % 16 == 0, (off * size) % 16 == 0, pad == 0) for name, (pad, off) in
                   ((nm, lay.LAYOUTS[nm][prec]) for nm in lay.LAYOUTS)}
            assert geo["D"][1:] == (True, True) and geo["O1"][1:] == (False, True)
            assert geo["RA"] == ((k * size) % 16 == 0, True, False)  # as aligned as dense rows of k are, and ld != k
            assert geo["R1"][1:] == (True, False) and geo["RO"][1:] == (False, False)
        # k = 16: O1 is the only unaligned base at a stride of whole 16 bytes; RA the only such stride with ld != k
        at16 = {name: ((16 + pad) * size % 16, off * size % 16, pad) for name, (pad, off) in ((nm, lay.LAYOUTS[nm][prec]) for nm in lay.LAYOUTS)}
        assert [nm for nm, (s, o, _) in at16.items() if s == 0 and o != 0] == ["O1"]
        assert [nm for nm, (s, o, pad) in at16.items() if s == 0 and o == 0 and pad] == ["RA"]
        assert all(s != 0 for nm, (s, _, _) in at16.items() if nm in ("R1", "RO"))


def test_every_layout_occurs_on_each_side_of_the_pair_list():
    assert len(lay.PAIRS) == len(set(lay.PAIRS)) == 9 and lay.CONTROL == ("D", "D") and lay.CONTROL not in lay.PAIRS
    assert {a for a, _ in lay.PAIRS} == set(lay.LAYOUTS) == {b for _, b in lay.PAIRS}
    for x, y in (("RA", "R1"), ("RA", "O1")):                            # aligned with a stride meets unaligned, in both directions
        assert (x, y) in lay.PAIRS and (y, x) in lay.PAIRS
    for prec in ("f32", "f64"):
        assert lay.LAYOUTS["D"][prec] == (0, 0)
        assert len({lay.LAYOUTS[nm][prec] for nm in lay.LAYOUTS}) == len(lay.LAYOUTS)


# ---- the special values of test_hip_factor_layouts.py::test_special_values_inside_a_strided_layout ------------------------------------
# Problem S of tests/test_hip_sweep_rows.py, one value at column 0 and one at column k - 1 of the first and of the last row of A and of B.
# A NaN or an infinity in a row of B makes the score of that item non-finite for every user who does not hold it as a train item, and
# the reference then declares the whole user NaN: such a value in B would turn (nearly) everybody into NaN, and the case would show
# nothing.  So the rows of A take NaN, +Inf and the large finite value, the rows of B the large finite value: LARGE x the largest
# factor of the other matrix x k is beyond the bound of scores_may_overflow (3.0e38 / 1.0e308), while every score stays finite (a score
# of item 0 or n - 1 is at most 2 x LARGE x max|A| in magnitude).
LARGE = {"f32": np.float32(5e37), "f64": np.float64(2e307)}
OVERFLOW_BOUND = {"f32": 3.0e38, "f64": 1.0e308}
K_SPECIAL = 5
SPECIAL_FACTORS = 16


@functools.lru_cache(maxsize=None)
def special_problem(prec, factors=SPECIAL_FACTORS):
    pr = problem(prec, factors)
    A, B = pr["A"].copy(), pr["B"].copy()
    big = LARGE[prec]
    A[0, 0], A[0, -1], A[-1, 0], A[-1, -1] = np.nan, np.inf, np.inf, big
    B[0, 0], B[0, -1], B[-1, 0], B[-1, -1] = big, -big, -big, big
    return dict(pr, A=A, B=B)


def users_that_change(oracle, prec, request):
    dtype = DTYPE[prec]
    outs = []
    for pr in (problem(prec, SPECIAL_FACTORS), special_problem(prec)):
        outs.append(oracle.calc(pr["A"], pr["B"], pr["train"], pr["test"], K_SPECIAL, metrics=request, cumulative=True, dtype=dtype, nthreads=NT))
    clean, planted = outs
    changed = ~np.all([same_bits(clean[nm], planted[nm]).reshape(M_USERS, -1).all(axis=1) for nm in clean], axis=0)
    nan_users = np.all([np.isnan(planted[nm]).reshape(M_USERS, -1).all(axis=1) for nm in planted], axis=0)
    return changed, nan_users


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_special_values_change_somebody_and_not_everybody(oracle, prec):
    """On the oracle alone.  The top-K request: at least one user changes in a bit against the clean problem, at most half of the users
    do (an item whose score jumps to the top or the bottom of a list of 5 moves a test item of that list for a minority).  With
    ROC / PR-AUC in the request such an item shifts a rank sum of nearly everybody, so "at most half change" cannot hold there; what
    keeps a kernel that turned everybody into NaN from passing is then stated directly: at most half of the users are NaN."""
    pr, clean = special_problem(prec), problem(prec, SPECIAL_FACTORS)
    k = pr["A"].shape[1]
    amax = lambda X: float(np.abs(X[np.isfinite(X)]).max())
    assert k * amax(clean["A"]) * float(LARGE[prec]) * 1.001 >= OVERFLOW_BOUND[prec]          # the finite value alone breaks the bound
    assert np.isfinite(pr["B"]).all() and 2 * float(LARGE[prec]) * amax(clean["A"]) < float(np.finfo(DTYPE[prec]).max) / 2
    changed, nan_users = users_that_change(oracle, prec, TOPK8)
    assert changed[0] and nan_users[0]                                    # the NaN in A's first row
    assert 1 <= changed.sum() <= M_USERS // 2, changed.sum()
    assert nan_users.sum() <= len(NO_TEST_USERS) + 1                       # user 0 and the users without test items, nobody else
    changed_all, nan_all = users_that_change(oracle, prec, ALL)
    assert changed_all.sum() >= changed.sum() and (nan_all == nan_users).all() and nan_all.sum() <= M_USERS // 2
