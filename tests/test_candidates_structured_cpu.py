"""CPU only: the rows and factors of tests/test_hip_candidates_structured.py reach the branches of k_topk_candidates they are meant for.

_candidates.schedule -- a model of the schedule the comment at the head of csrc/rm_candidates.hpp promises -- is run on the oracle's
scores of the very arrays the GPU module hands to the device (the case tables are _candidates.py's, imported by both), and its counts
are asserted: compactions, appends behind a bound, bounds inside a run of ties, idle wavefront steps in front of and behind live ones.
The model itself is held against the checker: its surviving pairs, ordered, are expected_lists' list for every user of every case."""
import numpy as np
import pytest

import _candidates as cs
from _candidates import CAND_STEP, CAP, F32, rows_of, schedule, scores_of, want_of
from _util import assert_same_bits

NAME = {np.float32: "f32", np.float64: "f64"}


def _schedules(family, K, *args, cand=None):
    case = cs.FAMILIES[family](*args)
    S = scores_of(family, *args)
    return [schedule(r, S[u], K) for u, r in enumerate(rows_of(case["cand"] if cand is None else cand))]


def _model_equals_checker(sch, want, what):
    """the model's survivors against expected_lists on the complement: every user"""
    ids, sc, st = want
    K = ids.shape[1]
    for u, s in enumerate(sch):
        assert s["status"] == st[u], "%s: user %d status %d, the checker says %d" % (what, u, s["status"], st[u])
        c = s["ids"].shape[0]
        assert (ids[u, :c] == s["ids"]).all() and (ids[u, c:] == -1).all(), "%s: user %d" % (what, u)
        assert_same_bits(sc[u, :c], s["scores"], "%s: user %d" % (what, u))
        assert np.isnan(sc[u, c:]).all() and c == (min(K, s["live"]) if st[u] == 0 else 0)


@pytest.mark.parametrize("K", cs.ORDER_K)
@pytest.mark.parametrize("kind,dtype,kf", cs.ORDER_CASES, ids=["%s-%s-k%d" % (kind, NAME[d], kf) for kind, d, kf in cs.ORDER_CASES])
def test_order_along_long_rows(kind, dtype, kf, K):
    sch = _schedules("order", K, kind, dtype, kf)
    want = want_of("order", K, kind, dtype, kf)
    _model_equals_checker(sch, want, kind)
    counts = np.array(cs.ORDER_COUNTS)
    assert [s["longrow"] for s in sch] == (counts > CAP).tolist() and [s["live"] for s in sch] == counts.tolist()
    assert all(s["compactions"] == 0 for s in sch[:1] + sch[len(cs.ORDER_LONG):])          # 2,048 entries and fewer: append everything
    assert all(s["compactions"] >= 1 for s in sch[1:len(cs.ORDER_LONG)])
    long = [u for u in range(cs.ORDER_M) if sch[u]["longrow"]]
    if kind == "ascending":
        assert all(sch[u]["appends"] == sch[u]["live"] for u in range(cs.ORDER_M))
        # 6,000 entries, 24 steps: the first compaction in front of step 8 (8 x 256 + 256 > 2,048), then every 7 steps with K = 10
        # (10 + 7 x 256 + 256 > 2,048: steps 15, 22) and every 4 with K = 1,024 (steps 12, 16, 20)
        full = sch[cs.ORDER_COUNTS.index(6000)]
        assert full["compactions"] == {1: 3, 10: 3, 1024: 4}[K]
    if kind == "descending":
        assert all(sch[u]["appends_after"] == 0 for u in long)
    if kind == "trend" and K == 10:
        # test_structured_cpu.py's criterion: at least ten times the i.i.d. row's appends behind the first bound (K = 10: with K =
        # 1,024 an i.i.d. row already appends a quarter of what is left, and ten times that is more than the row holds)
        S = scores_of("order", "iid", dtype, kf)                  # (the same candidate rows, synth.make_factors)
        cand = cs.order_case(kind, dtype, kf)["cand"]
        for u in (cs.ORDER_COUNTS.index(4999), cs.ORDER_COUNTS.index(6000)):
            iid = schedule(rows_of(cand)[u], S[u], K)["appends_after"]
            print("trend, %s, %d entries: %d appends behind the first compaction, i.i.d. %d" % (NAME[dtype], cs.ORDER_COUNTS[u], sch[u]["appends_after"], iid))
            assert iid >= 1 and sch[u]["appends_after"] >= 10 * iid
    if kind == "blocks":
        assert all(sch[u]["bound_in_tie"] for u in long)             # 20 distinct scores per user: every bound lies inside a block
    if kind == "runs" and K > 1:
        assert any(sch[u]["bound_in_tie"] for u in long)
    if kind == "equal":
        for u, r in enumerate(rows_of(cs.order_case(kind, dtype, kf)["cand"])):
            assert (want[0][u, :min(K, r.shape[0])] == r[:K]).all() and len(set(want[1][u, :min(K, r.shape[0])].tolist())) == 1


@pytest.mark.parametrize("K", cs.DUP_K)
@pytest.mark.parametrize("dtype,kf", cs.DUP_CASES, ids=["%s-k%d" % (NAME[d], kf) for d, kf in cs.DUP_CASES])
def test_duplicates_at_scale(dtype, kf, K):
    case = cs.duplicate_case(dtype, kf)
    sch = _schedules("duplicates", K, dtype, kf)
    _model_equals_checker(sch, want_of("duplicates", K, dtype, kf), "duplicates")
    # the shuffled rows are the same sets: the plan stage sorts them, and the kernel sees the rows above
    for a, b in zip(rows_of(cs.shuffled(case["cand"], 5)), rows_of(case["cand"])):
        assert (np.sort(a) == b).all()
    by = {name: s for name, s in zip(case["names"], sch)}
    runs = {name: s for name, s in by.items() if name[0] == "dup_run"}
    assert len(runs) == 42 and {name[3] for name in runs} == set(cs.DUP_TIMES)
    for name, s in runs.items():
        assert s["live"] == name[1] and s["longrow"] == (name[1] + name[3] - 1 > CAP)
        if name[3] >= 128:
            assert s["idle"], name
    assert any(s["idle_then_live"] for s in runs.values()) and any(s["live_then_idle"] for s in runs.values())
    for name, s in runs.items():
        if name[3] == 2100:                                          # a whole step of duplicates, live steps on both sides (or the row's end)
            steps = -(-(name[1] + 2099) // CAND_STEP)
            assert s["idle_steps"] and s["longrow"] and min(s["idle_steps"]) > 0, name
            if name[2] < name[1] - 1:
                assert max(s["idle_steps"]) < steps - 1, name
    assert any(name[3] == 2100 and name[2] < name[1] - 1 for name in runs)
    assert by[("one_id",)]["live"] == 1 and by[("one_id",)]["longrow"] and len(by[("one_id",)]["idle_steps"]) == 5000 // CAND_STEP
    few = by[("few_distinct",)]
    assert few["longrow"] and few["live"] == 500 < 1024 and few["compactions"] == 0
    assert (by[("2048 entries, 2047 distinct",)]["longrow"], by[("2049 entries, 2048 distinct",)]["longrow"]) == (False, True)
    assert by[("2049 entries, 2048 distinct",)]["compactions"] == 1
    assert by[("empty",)]["status"] == 1
    rows = rows_of(case["cand"])
    chain = [u for u, name in enumerate(case["names"]) if name[0] == "chained"]
    assert len(chain) == 4 and np.diff(chain).tolist() == [1, 1, 1]
    for u in chain[:-1]:
        assert rows[u + 1][0] == rows[u][-1] and (rows[u][-70:] == rows[u][-1]).all() and rows[u][-71] != rows[u][-1]
        assert sch[u + 1]["live"] <= min(cs.DUP_K)                   # every id is in the list: a first entry taken for a duplicate is missed


@pytest.mark.parametrize("K", cs.NF_K)
@pytest.mark.parametrize("order,dtype", cs.NF_CASES, ids=["%s-%s" % (o, NAME[d]) for o, d in cs.NF_CASES])
def test_non_finite_scores_in_long_rows(order, dtype, K):
    case = cs.nonfinite_case(order, dtype)
    sch = _schedules("nonfinite", K, order, dtype)
    want = want_of("nonfinite", K, order, dtype)
    _model_equals_checker(sch, want, order)
    assert set(np.flatnonzero(want[2] == 2).tolist()) == set(case["hit"]) and set(want[2].tolist()) == {0, 2}
    assert len(case["hit"]) == (6 if order == "ascending" else 1)
    assert (want[0][want[2] == 2] == -1).all() and np.isnan(want[1][want[2] == 2]).all()
    rows, S = rows_of(case["cand"]), scores_of("nonfinite", order, dtype)
    assert all(r.shape[0] == cs.NF_ENTRIES for r in rows) and all(s["longrow"] and s["compactions"] >= 1 for s in sch)
    assert not any(cs.NF_UNLISTED in r for r in rows) and np.isnan(S[:, cs.NF_UNLISTED]).all()
    for u, item in case["items"].items():
        at = int(np.searchsorted(rows[u], item))
        assert rows[u][at] == item and [v for v in range(cs.NF_M) if item in rows[v]] == [u]
        what = case["hit"][u]
        if "first step" in what:
            assert at < CAND_STEP and np.isnan(S[u, item])
        if "second compaction" in what:
            assert at >= cs.NF_SECOND_COMPACTION and np.isnan(S[u, item]) and schedule(rows[u][:at], S[u], K)["compactions"] >= 2
        if "last" in what:
            assert at == cs.NF_ENTRIES - 1
        if "-Inf" in what:
            # far below the bound: never appended -- only the statistics see it
            clean = schedule(rows[u][:-1], S[u], K)
            assert S[u, item] == -np.inf and clean["status"] == 0 and S[u, item] < clean["scores"][-1] and sch[u]["appends_after"] == 0
        if "+Inf" in what:
            assert S[u, item] == np.inf
    if order == "ascending":
        u, item = case["overflow"]
        assert np.isfinite(case["A"][u]).all() and np.isfinite(case["B"][item]).all() and case["A"][u, 0] >= 1 and S[u, item] == np.inf


@pytest.mark.parametrize("dtype,kf", cs.COUNTS_CASES, ids=["%s-k%d" % (NAME[d], kf) for d, kf in cs.COUNTS_CASES])
def test_factor_counts_over_several_steps(dtype, kf):
    sch = _schedules("counts", cs.COUNTS_K, dtype, kf)
    _model_equals_checker(sch, want_of("counts", cs.COUNTS_K, dtype, kf), "%d factors" % kf)
    assert [s["live"] for s in sch] == list(cs.COUNTS_ROWS) and {257, 600, 2305} <= set(cs.COUNTS_ROWS)
    assert sch[cs.COUNTS_ROWS.index(2305)]["compactions"] == 1            # in front of step 8; step 9 appends behind the bound


def test_batch_and_shard_edges():
    case = cs.edge_case()
    sch = _schedules("edges", cs.EDGE_K)
    want = want_of("edges", cs.EDGE_K)
    _model_equals_checker(sch, want, "edges")
    assert case["A"].dtype == F32 and set(want[2].tolist()) == {0, 1}
    # the last user of a batch of 1,024 and the first of the next; the last user of each of three shards of 700
    assert set(case["kinds"]) == {1023, 1024, 2047, 2048, cs.EDGE_M // 3 - 1, 2 * cs.EDGE_M // 3 - 1, cs.EDGE_M - 1} and cs.EDGE_M % 3 == 0
    assert set(case["kinds"].values()) == set(cs.EDGE_ROWS)
    for u, kind in case["kinds"].items():
        s = sch[u]
        if kind == "long":
            assert s["live"] == 2305 and s["compactions"] == 1 and s["appends"] == 2305          # (ascending: everything is appended)
        if kind == "dup_run":
            assert s["idle"] and s["idle_then_live"]
        if kind == "few_distinct":
            assert s["longrow"] and s["live"] == 500
        if kind == "empty":
            assert s["status"] == 1
    others = [s for u, s in enumerate(sch) if u not in case["kinds"]]
    assert max(s["live"] for s in others) <= 8 and any(s["status"] == 1 for s in others)
