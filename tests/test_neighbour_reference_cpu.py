"""tests/neighbour_reference.py against the known answers of the reference's ItemKNN tests
(tests/golden/neighbour_known_answers.json) and against cases worked by hand: ties in both directions, duplicated rows,
a zero denominator, the inner join."""
import json
import math
from pathlib import Path

import numpy as np
import pytest

import neighbour_reference as NR

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "neighbour_known_answers.json").read_text())


def columns(rows):
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def fit(case, weighting, k=1):
    user, item, rel = columns(case["rows"])
    w = NR.weights(user, item, rel, False, weighting)
    n_users, n_items = max(user) + 1, max(item) + 1
    return user, item, w, NR.table(*NR.similarity(user, item, w, n_users, n_items, k))


def test_known_answers_of_the_plain_model():
    case = GOLDEN["log"]
    user, item, w, sim = fit(case, None)
    assert list(w) == [1.0] * 4
    # 1 / (sqrt(2) * sqrt(2)): the rounded product of the two rounded roots is 2 (1 + 2^-52), so 0.5 holds to an ulp
    assert sim == {0: [(1, 1.0 / (math.sqrt(2.0) * math.sqrt(2.0)))], 1: [(0, 1.0 / (math.sqrt(2.0) * math.sqrt(2.0)))]}
    assert sim[0][0][1] == pytest.approx(case["similarity_0_1"], rel=2.0 ** -51)
    assert sim[1][0][1] == pytest.approx(case["similarity_1_0"], rel=2.0 ** -51)
    recs = NR.predict(sim, user, item, case["users"], [0, 1], case["k"])
    assert {str(u): r[0][0] for u, r in recs.items()} == case["recommended"]
    assert recs[0] == sim[0] and recs[1] == sim[1]


def test_known_answers_of_tf_idf():
    case = GOLDEN["weighting_log"]
    user, item, w, sim = fit(case, "tf_idf")
    for u, x in zip(user, w):
        assert x == pytest.approx(case["tf_idf"]["idf"][str(u)], rel=1e-15)
    recs = NR.predict(sim, user, item, case["users"], [0, 1], case["k"])
    assert recs[1][0][0] == case["tf_idf"]["recommended"]["1"]
    assert recs[0] == []                                   # user 0 has seen both items


def test_known_answers_of_bm25():
    case = GOLDEN["weighting_log"]
    assert (NR.BM25_K1, NR.BM25_B) == (case["bm25_k1"], case["bm25_b"])
    user, item, w, sim = fit(case, "bm25")
    for u, i, x in zip(user, item, w):
        assert x == pytest.approx(case["bm25"]["tf"][str(i)] * case["bm25"]["idf"][str(u)], rel=1e-14)
    recs = NR.predict(sim, user, item, case["users"], [0, 1], case["k"])
    assert recs[1][0][0] == case["bm25"]["recommended"]["1"]
    with pytest.raises(ValueError, match="weighting must be one of"):
        NR.weights(user, item, None, False, " ")


def test_relevance_is_used_only_when_asked_for():
    user, item, rel = [0, 0, 1], [0, 1, 1], [0.5, -2.0, 0.0]
    assert list(NR.weights(user, item, rel, False)) == [1.0, 1.0, 1.0]
    assert list(NR.weights(user, item, rel, True)) == rel
    assert NR.norms(item, rel, 3) == [0.5, 2.0, 0.0]


def test_the_product_is_an_inner_join_and_a_zero_sum_is_a_candidate():
    L = [[(0, 1.0), (1, 1.0)], [], [(2, 1.0)]]
    R = [[(0, 1.0), (2, 0.5)], [(0, -1.0)], []]
    terms = NR.product(L, R)
    assert terms == [{0: [1.0, -1.0], 2: [0.5]}, {}, {}]
    ids, vals, count = NR.topk(L, R, 3, NR.PREDICT)
    assert ids.tolist() == [[2, 0, -1], [-1, -1, -1], [-1, -1, -1]] and count.tolist() == [2, 0, 0]
    assert vals.tolist() == [[0.5, 0.0, 0.0], [0.0] * 3, [0.0] * 3]          # column 0 is reached and sums to 0; 1 is not


def test_ties_go_down_for_fit_and_up_for_predict():
    L = [[(0, 1.0)], [(0, 1.0)]]
    R = [[(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0)]]
    ones = [1.0] * 4
    ids, vals, count = NR.topk(L, R, 3, NR.FIT, ones, ones, 1.0)
    assert ids.tolist() == [[3, 2, 1], [3, 2, 0]] and count.tolist() == [3, 3] and vals.tolist() == [[0.5] * 3] * 2
    ids, vals, count = NR.topk(L, R, 3, NR.PREDICT)
    assert ids.tolist() == [[0, 1, 2], [0, 1, 2]] and vals.tolist() == [[1.0] * 3] * 2
    ids, _, count = NR.topk(L, R, 3, NR.PREDICT, mask=[0, 1, 1, 1], seen=[[1], [1, 2, 3]])
    assert ids.tolist() == [[2, 3, -1], [-1, -1, -1]] and count.tolist() == [2, 0]


def test_zero_denominators_are_dropped_and_shrink_brings_them_back():
    user, item, w = [0, 0, 0], [0, 1, 2], [1.0, 0.0, 2.0]                    # item 1 has norm 0
    ids, vals, count = NR.similarity(user, item, w, 1, 3, 2)
    assert ids.tolist() == [[2, -1], [-1, -1], [0, -1]] and count.tolist() == [1, 0, 1] and vals[0, 0] == 1.0
    ids, vals, count = NR.similarity(user, item, w, 1, 3, 2, shrink=2.0)
    assert ids.tolist() == [[2, 1], [2, 0], [0, 1]] and vals.tolist() == [[0.5, 0.0], [0.0, 0.0], [0.5, 0.0]]


def test_duplicated_rows_never_pair_an_item_with_itself_and_count_twice_against_others():
    user, item, w = [0, 0, 0], [0, 0, 1], [1.0, 1.0, 1.0]
    ids, vals, count = NR.similarity(user, item, w, 1, 2, 5)
    assert count.tolist() == [1, 1] and ids[:, 0].tolist() == [1, 0]
    assert vals[0, 0] == 2.0 / (math.sqrt(2.0) * 1.0) and vals[1, 0] == vals[0, 0]
    sim = NR.table(ids, vals, count)
    recs = NR.predict(sim, user, item, [0, 7], [0, 1], 5, filter_seen_items=False)
    assert recs[7] == [] and recs[0] == [(1, 2 * vals[0, 0]), (0, vals[0, 0])]  # two log rows of item 0 both vote for 1
    assert NR.pair_scores(sim, user, item, [(0, 1), (0, 0), (0, 5), (7, 1)]) == [2 * vals[0, 0], vals[0, 0], None, None]
    assert NR.predict(sim, user, item, [0], [1], 5, filter_seen_items=True) == {0: []}


def test_tolerances():
    assert NR.tolerance("weight", 2.0) == 8 * 2.0 ** -52
    assert NR.tolerance("similarity", 0.5, terms=3, n_i=4, n_j=5) == 20 * 2.0 ** -53 * 0.5
    assert NR.tolerance("score", terms=3, sum_abs=2.0) == 6 * 2.0 ** -53
    with pytest.raises(ValueError):
        NR.tolerance("other")


def test_csr_of_rows():
    off, col, val = NR.csr([[(3, 1.5)], [], [(0, 2.0), (1, -1.0)]])
    assert off.tolist() == [0, 1, 1, 3] and col.tolist() == [3, 0, 1] and val.tolist() == [1.5, 2.0, -1.0]
    assert (off.dtype, col.dtype, val.dtype) == (np.int64, np.int32, np.float64)
