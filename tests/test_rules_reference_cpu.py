"""The yardstick of the association rules (tests/rules_reference.py) without a GPU: it reproduces the known answers of
tests/golden/association_rules_known_answers.json, its mirrored measures are consistent, and on the crafted logs of the
GPU tests every plausible mistake -- a duplicate kept, the product in place of the minimum, either threshold off by one,
ties the other way round -- changes its output: a device that made one of them would not pass tests/test_gpu_rules.py."""
import json
import math
from pathlib import Path

import numpy as np
import pytest

import neighbour_reference as NR
import rules_reference as RR

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "association_rules_known_answers.json").read_text())
_CACHE = {}


def log(name):
    if name not in _CACHE:
        _CACHE[name] = getattr(RR, name)()
    return _CACHE[name]


def rows_of(table):
    ids, conf, lift, gain, count = table
    return [{"item_idx_one": a, "item_idx_two": int(ids[a, r]), "confidence": conf[a, r], "lift": lift[a, r],
             "confidence_gain": gain[a, r]} for a in range(len(count)) for r in range(count[a])]


def differs(a, b):
    return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


def test_the_docstring_log():
    case = GOLDEN["docstring"]
    lg = case["log"]
    table = RR.table(lg["user_idx"], lg["item_idx"], lg["relevance"], 4, None, **case["args"])
    assert rows_of(table) == case["similarity"]
    pairs = list(zip(case["predict_pairs"]["pairs"]["user_idx"], case["predict_pairs"]["pairs"]["item_idx"]))
    for plane, metric in ((1, "confidence"), (2, "lift")):
        sim = NR.table(table[0], table[plane], table[4])
        assert NR.pair_scores(sim, lg["user_idx"], lg["item_idx"], pairs) == case["predict_pairs"][metric]


def test_the_fixture_log_plain_and_with_relevance():
    case = GOLDEN["fixture"]
    lg = case["log"]
    for key, use in (("plain", False), ("use_relevance", True)):
        want = case[key]
        rows = RR.distinct_rows(lg["user_idx"], lg["item_idx"], lg["relevance"], use)
        count, rel, n = RR.item_stats(rows)
        assert len(rows) == want["distinct_rows"] and n == case["num_sessions"]
        a, b = want["pair"]
        terms = RR.pairs(rows, set(count))[a, b]
        assert [rel[a], rel[b], math.fsum(terms)] == want["counts"]
        table = RR.table(lg["user_idx"], lg["item_idx"], lg["relevance"], 4, None, use_relevance=use, **case["args"])
        row = [r for r in rows_of(table) if (r["item_idx_one"], r["item_idx_two"]) == (a, b)]
        assert len(row) == 1 and {m: row[0][m] for m in RR.METRICS} == want["expected"]
    table = RR.table(lg["user_idx"], lg["item_idx"], lg["relevance"], 4, None, **case["args"])
    for q in case["nearest"]:
        found = [r for r in rows_of(table) if r["item_idx_one"] in q["items"] and
                 (q["candidates"] is None or r["item_idx_two"] in q["candidates"])]
        assert len(found) == q["rows"]
        if "values" in q:
            assert [r[q["metric"]] for r in found] == q["values"]


def test_rejected_relevances_and_signed_zero():
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="NaN or an infinite"):
            RR.distinct_rows([0, 0], [1, 2], [1.0, bad], True)
    assert RR.distinct_rows([0, 0], [1, 2], [1.0, math.nan], False) == [(0, 1, 1.0), (0, 2, 1.0)]
    assert len(RR.distinct_rows([0, 0, 0], [1, 1, 1], [0.0, -0.0, 0.5], True)) == 2


@pytest.mark.parametrize("name,use", [("count_log", False), ("dyadic_log", True)])
def test_mirrored_measures_are_consistent(name, use):
    session, item, rel, n_items = log(name)
    rows = RR.distinct_rows(session, item, rel, use)
    _, item_rel, n = RR.item_stats(rows)
    ids, conf, lift, gain, count = RR.table(session, item, rel, n_items, None, 1, 1, use)
    at = {(a, int(ids[a, r])): r for a in range(n_items) for r in range(count[a])}
    assert at and all((b, a) in at for a, b in at)                                # the pair filter is symmetric
    for (a, b), r in at.items():
        back = at[b, a]
        assert lift[a, r] == pytest.approx(lift[b, back], rel=8 * RR.EPS)        # n p / (A C) either way
        assert conf[a, r] * item_rel[a] == pytest.approx(conf[b, back] * item_rel[b], rel=8 * RR.EPS)
        assert a != b and not math.isnan(gain[a, r])
        if gain[a, r] == math.inf:                                                # C - p == 0: p = confidence * A = C
            assert conf[a, r] * item_rel[a] == pytest.approx(item_rel[b], rel=8 * RR.EPS)
    for a in range(n_items):                                                      # lift descending, then id descending
        keys = [(-(lift[a, r] + 0.0), -int(ids[a, r])) for r in range(count[a])]
        assert keys == sorted(keys)


def test_each_mistake_shows_on_the_crafted_logs():
    session, item, rel, n_items = log("count_log")
    for k in (1, 3, 10):
        for pair_min in (1, 3):
            for item_min in (1, 4):
                args = (session, item, rel, n_items, k, item_min, pair_min)
                good = RR.table(*args)
                assert differs(good, RR.table(*args, dedup=False)), "a duplicate kept"
                assert differs(good, RR.table(*args, tie_desc=False)), "ties by the smaller id"
                for slack in (-1, 1):
                    if k == 10 and pair_min + slack >= 1:                     # thresholds 0 and 1 keep the same pairs
                        assert differs(good, RR.table(*args, pair_slack=slack)), "pair threshold off by one"
                    if k == 10 and item_min + slack >= 1 and (item_min == 4 or pair_min == 1):   # one row: no pair of 3
                        assert differs(good, RR.table(*args, item_slack=slack)), "item threshold off by one"
    session, item, rel, n_items = log("dyadic_log")
    args = (session, item, rel, n_items, 10, 1, 1, True)
    good = RR.table(*args)
    assert differs(good, RR.table(*args, combine=lambda a, b: a * b)), "the product in place of the minimum"
    assert differs(good, RR.table(*args, dedup=False)), "a duplicate kept"
    assert differs(good, RR.table(session, item, rel, n_items, 10, 1, 1, False)), "the relevance ignored"


def test_the_crafted_logs_hold_what_their_docstrings_say():
    session, item, rel, n_items = log("count_log")
    assert len(set(session.tolist())) == 300 and n_items == 60 and int(item.max()) == 59
    rows = RR.distinct_rows(session, item, rel)
    assert len(rows) < len(session)                                               # duplicated rows
    count, _, n = RR.item_stats(rows)
    terms = {ab: len(t) for ab, t in RR.pairs(rows, set(count)).items()}
    assert n == 300 and [count[i] for i in (48, 49, 50, 51, 52)] == [1, 2, 3, 4, 5]
    assert [terms[53, b] for b in (54, 55, 56)] == [2, 3, 4]
    best = RR.table(session, item, rel, n_items, 2, 1, 1)
    assert best[0][57].tolist() == [59, 58] and best[2][57, 0] == best[2][57, 1] == 300 / 6
    session, item, rel, n_items = log("dyadic_log")
    assert np.array_equal(rel * 8, np.round(rel * 8)) and np.abs(rel).max() <= 16.0
    rows = RR.distinct_rows(session, item, rel, True)
    count, item_rel, _ = RR.item_stats(rows)
    terms = {ab: len(t) for ab, t in RR.pairs(rows, set(count)).items()}
    assert [terms[a, a + 1] for a in (41, 43, 45, 47)] == [32, 33, 64, 65]
    assert item_rel[40] == 0 and count[40] == 6 and [r for r in rows if r[:2] == (0, 1)] == [(0, 1, 1.5), (0, 1, 3.0)]


def test_tolerance_is_the_stated_formula():
    assert RR.tolerance(3, 5, 2) == (3 + 5 + 2 + 4) * 2.0 ** -53
