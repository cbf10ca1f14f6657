"""Yardstick of the association rules (section f10 of include/cqlrec.h, replay_cql_amd/association_rules.py; DESIGN.md
section 3.13): plain Python over lists and dicts, written from the formulas and independent of the device code.

    distinct_rows  the distinct (session, item, w) triples of a log; -0.0 and +0.0 are one weight
    item_stats     rows and summed weight per item, and the number of sessions
    pairs          the terms min(w_a, w_b) of every ordered pair a != b that shares a session
    measures       confidence, lift and confidence gain of one pair, in the normative operation order
    table          the k best consequents per antecedent by (lift descending, id descending), all three measures
    tolerance      the relative bound the GPU test holds confidence and lift to on non-dyadic weights

Every sum is math.fsum: the correctly rounded sum of its terms, whatever their order.  Python floats are IEEE doubles,
so the three expressions of `measures` round exactly as the device's.  Prediction is neighbour_reference.predict /
pair_scores on `neighbour_reference.table(ids, plane, count)` of the chosen plane.

The keyword arguments of `table` after `use_relevance` exist for tests/test_rules_reference_cpu.py: each switches ONE
step to a plausible mistake, to show that the logs the GPU tests use tell the mistake from the rule."""
import math

import numpy as np

METRICS = ("confidence", "lift", "confidence_gain")
EPS = 2.0 ** -53


def distinct_rows(session, item, relevance=None, use_relevance=False, dedup=True):
    """[(session, item, w)] in ascending order, each distinct triple once; w = 1.0 or the row's relevance"""
    rows = []
    for r in range(len(session)):
        w = float(relevance[r]) + 0.0 if use_relevance else 1.0
        if math.isnan(w) or math.isinf(w):
            raise ValueError("relevance contains NaN or an infinite value")
        rows.append((int(session[r]), int(item[r]), w))
    return sorted(set(rows)) if dedup else sorted(rows)


def item_stats(rows):
    """({item: number of rows}, {item: fsum of their w}, number of distinct sessions)"""
    ws = {}
    for _, i, w in rows:
        ws.setdefault(i, []).append(w)
    return {i: len(v) for i, v in ws.items()}, {i: math.fsum(v) for i, v in ws.items()}, len({s for s, _, _ in rows})


def pairs(rows, items, combine=min):
    """{(a, b): [combine(w_a, w_b), ...]} over the row pairs of one session with a != b, both in `items`"""
    by_session = {}
    for s, i, w in rows:
        if i in items:
            by_session.setdefault(s, []).append((i, w))
    out = {}
    for rs in by_session.values():
        for a, wa in rs:
            for b, wb in rs:
                if a != b:
                    out.setdefault((a, b), []).append(combine(wa, wb))
    return out


def measures(p, A, C, n):
    """(confidence, lift, confidence_gain) of a pair with relevance p, antecedent relevance A, consequent relevance C
    and n sessions; A and C are non-zero"""
    n = float(n)
    confidence = p / A
    lift = (n * confidence) / C
    gain = math.inf if C - p == 0 else (confidence * (n - A)) / (C - p)
    return confidence, lift, gain


def table(session, item, relevance, n_items, k, min_item_count=5, min_pair_count=5, use_relevance=False, dedup=True,
          combine=min, item_slack=0, pair_slack=0, tie_desc=True):
    """(ids int32 [n_items, k] padded with -1, confidence, lift, confidence_gain float64 [n_items, k] padded with 0,
    count int32 [n_items]); k = None keeps every pair (k = n_items - 1)"""
    k = max(1, n_items - 1) if k is None else k
    rows = distinct_rows(session, item, relevance, use_relevance, dedup)
    count, rel, n = item_stats(rows)
    items = {i for i, c in count.items() if c >= min_item_count + item_slack}
    ids = np.full((n_items, k), -1, dtype=np.int32)
    planes = [np.zeros((n_items, k), dtype=np.float64) for _ in METRICS]
    cnt = np.zeros(n_items, dtype=np.int32)
    cand = {}
    for (a, b), terms in pairs(rows, items, combine).items():
        if len(terms) >= min_pair_count + pair_slack and rel[a] != 0 and rel[b] != 0:
            cand.setdefault(a, []).append((b, measures(math.fsum(terms), rel[a], rel[b], n)))
    sign = -1 if tie_desc else 1
    for a, lst in cand.items():
        best = sorted(lst, key=lambda bm: (-(bm[1][1] + 0.0), sign * bm[0]))[:k]
        cnt[a] = len(best)
        for r, (b, ms) in enumerate(best):
            ids[a, r] = b
            for plane, m in zip(planes, ms):
                plane[a, r] = m
    return (ids, *planes, cnt)


def term_counts(session, item, relevance, use_relevance=True):
    """({item: rows}, {(a, b): terms}) of the distinct rows: the lengths of the sums behind A, C and p"""
    rows = distinct_rows(session, item, relevance, use_relevance)
    count, _, _ = item_stats(rows)
    return count, {ab: len(t) for ab, t in pairs(rows, set(count)).items()}


def tolerance(n_a, n_b, n_ab):
    """Relative bound on |device - yardstick| of confidence and lift for non-negative weights: (n_a + n_b + n_ab + 4) *
    2^-53.  The three sums have n_ab, n_a and n_b terms of one sign, each summed in any order: first-order relative
    errors of at most n * 2^-53; confidence adds one rounding (the division), lift three (division, multiply,
    division); the yardstick's own fsum and roundings are within the + 4."""
    return (n_a + n_b + n_ab + 4) * EPS


# ------------------------------------------------------------------------------------------------- crafted logs
def _columns(rows):
    s, i, w = zip(*rows)
    return np.array(s, dtype=np.int64), np.array(i, dtype=np.int64), np.array(w, dtype=np.float64)


def count_log():
    """(session, item, relevance, n_items): 300 sessions x 60 items, count data with duplicated rows.  Items 0..47 are
    Zipf-distributed; the others are placed by hand, for min_item_count = 1 and 4 and min_pair_count = 1 and 3:
      48, 49           appear in 1 and 2 sessions: at and above the item threshold 1
      50, 51, 52       appear in 3, 4 and 5 sessions: below, at and above the item threshold 4
      53 with 54..56   co-occurs in 2, 3 and 4 sessions: below, at and above the pair threshold
      57, 58, 59       share the same 6 sessions, where nothing else is: equal lifts from every antecedent, and the
                       largest of all -- the cut of k = 1 falls inside the tie, and the larger id must win"""
    rng = np.random.default_rng(7)
    weight = 1.0 / np.arange(1, 49) ** 0.9
    weight /= weight.sum()
    rows = []
    for s in range(280):
        for i in rng.choice(48, size=int(rng.integers(2, 9)), p=weight):      # drawn with replacement: duplicates
            rows.append((s, int(i), 1.0))
    rows += rows[::5]                                                          # and every fifth row once more
    for i, sessions in ((48, (12,)), (49, (13, 14)), (50, range(0, 3)), (51, range(3, 7)), (52, range(7, 12)), (53, range(20, 30)), (54, (20, 21)),
                        (55, (22, 23, 24)), (56, (25, 26, 27, 28)), (57, range(280, 286)), (58, range(280, 286)),
                        (59, range(280, 286))):
        rows += [(s, i, 1.0) for s in sessions]
    rows += [(s, 10 + s % 7, 1.0) for s in range(286, 300)]
    order = np.random.default_rng(8).permutation(len(rows))
    return (*_columns([rows[r] for r in order]), 60)


def dyadic_log():
    """(session, item, relevance, n_items): 270 sessions x 50 items, relevances multiples of 2^-3 of magnitude <= 2^4, so
    every sum is exact.  Items 0..39 are random; by hand:
      (0, 1)           has the relevances 1.5 and 3.0, and the row (0, 1, 1.5) twice
      40               sums to 0 (0.0, -0.0 in one session, 2.0, -2.0, 0.0): its pairs are absent
      41/42 .. 47/48   co-occur in exactly 32, 33, 64 and 65 sessions: both reduction paths, at their boundaries
      42               weighs 1.0 wherever it is and 41 weighs more: C - p == 0, the gain of 41 -> 42 is +inf"""
    rng = np.random.default_rng(11)
    rows = []
    for s in range(200):
        for i in rng.choice(40, size=int(rng.integers(2, 8)), replace=False):
            rows.append((s, int(i), float(rng.integers(1, 129)) / 8.0))
    rows += [(0, 1, 1.5), (0, 1, 3.0), (0, 1, 1.5)]
    rows = [r for r in rows if not (r[0] == 0 and r[1] == 1 and r[2] not in (1.5, 3.0))]
    rows += [(1, 40, 0.0), (1, 40, -0.0), (2, 40, 2.0), (3, 40, -2.0), (4, 40, 0.0), (5, 40, 0.0), (6, 40, 0.0)]
    for a, n in ((41, 32), (43, 33), (45, 64), (47, 65)):
        for s in range(200, 200 + n):
            rows.append((s, a, float(rng.integers(8, 129)) / 8.0))
            rows.append((s, a + 1, 1.0 if a == 41 else float(rng.integers(1, 129)) / 8.0))
    rows += [(s, 49, 0.125) for s in range(265, 270)] + [(s, 41, 16.0) for s in range(265, 270)]
    order = np.random.default_rng(12).permutation(len(rows))
    return (*_columns([rows[r] for r in order]), 50)
