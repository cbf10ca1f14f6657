"""Yardstick of the neighbourhood models (section f8 of include/cqlrec.h, replay_cql_amd/neighbour.py): plain Python /
numpy over lists and dicts, written from the semantics and independent of the device code.

    weights      the weight of every log row: 1 or the relevance, tf-idf, bm25
    norms        sqrt(sum of w^2) per item
    product      the terms of every reached (row, j) of a sparse x sparse product
    topk         both epilogues (FIT, PREDICT) and the k best per row
    similarity   ItemKNN.fit: the k most similar items of every item
    predict      NeighbourRec.predict: the k best items per user from a similarity table
    pair_scores  NeighbourRec.predict_pairs
    tolerance    the bounds the GPU tests hold the device to, with their derivations

Every sum is math.fsum: the correctly rounded sum of its terms, whatever their order.  Each function takes what the step
before it made, so a test can feed in what the device produced (its weights, its similarity table)."""
import math

import numpy as np

FIT, PREDICT = 0, 1
BM25_K1, BM25_B = 1.2, 0.75
EPS = 2.0 ** -53


def weights(user, item, relevance=None, use_relevance=False, weighting=None, k1=BM25_K1, b=BM25_B):
    """float64 [n_rows].  DF = rows of the user, cnt = rows of the item, n_items = distinct items, avgdl = n_rows / n_items."""
    user, item = np.asarray(user, dtype=np.int64), np.asarray(item, dtype=np.int64)
    n = len(user)
    rel = np.asarray(relevance, dtype=np.float64).copy() if use_relevance else np.ones(n, dtype=np.float64)
    if weighting is None or n == 0:
        return rel
    if weighting not in ("tf_idf", "bm25"):
        raise ValueError("weighting must be one of [None, 'tf_idf', 'bm25']")
    df = np.bincount(user)[user].astype(np.float64)
    cnt = np.bincount(item)[item].astype(np.float64)
    n_items = float(len(np.unique(item)))
    if weighting == "tf_idf":
        return rel * np.log1p(n_items / df)
    avgdl = float(n) / n_items
    tf = rel * (k1 + 1.0) / (rel + k1 * (1.0 - b + b * (cnt / avgdl)))
    return tf * np.log1p((n_items - df + 0.5) / (df + 0.5))


def norms(item, w, n_items):
    sq = [[] for _ in range(n_items)]
    for i, x in zip(item, w):
        sq[int(i)].append(float(x) * float(x))
    return [math.sqrt(math.fsum(s)) for s in sq]


def csr(rows):
    """(offsets int64, cols int32, vals float64) of a list of rows, each a list of (column, value)"""
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    for q, r in enumerate(rows):
        off[q + 1] = off[q] + len(r)
    col = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    val = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return off, col, val


def product(L, R):
    """[per row of L] {j: [a * b, ...]} over the entries (m, a) of the row and (j, b) of R[m]: an inner join, so a j no
    combination reaches is absent, and a reached j keeps every one of its terms"""
    out = []
    for row in L:
        terms = {}
        for m, a in row:
            if m < len(R):
                for j, b in R[m]:
                    terms.setdefault(int(j), []).append(float(a) * float(b))
        out.append(terms)
    return out


def candidates(terms, mode, q, norm_q=None, norm_j=None, shrink=0.0, mask=None, seen=None):
    """{j: value} of one row after the epilogue"""
    out = {}
    for j, ts in terms.items():
        c = math.fsum(ts)
        if mode == FIT:
            den = float(norm_q[q]) * float(norm_j[j]) + float(shrink)
            if j == q or den == 0.0:
                continue
            out[j] = c / den
        else:
            if mask is not None and not mask[j]:
                continue
            if seen is not None and j in seen:
                continue
            out[j] = c
    return out


def order(cand, mode):
    """[(j, value)] by value descending, then j descending (FIT) or ascending (PREDICT)"""
    sign = -1 if mode == FIT else 1
    return sorted(cand.items(), key=lambda kv: (-kv[1], sign * kv[0]))


def topk(L, R, k, mode, norm_q=None, norm_j=None, shrink=0.0, mask=None, seen=None):
    """(ids int32 [n_q, k] padded with -1, vals float64 [n_q, k] padded with 0, count int32 [n_q]); seen: None or one
    collection of columns per row"""
    n_q = len(L)
    ids = np.full((n_q, k), -1, dtype=np.int32)
    vals = np.zeros((n_q, k), dtype=np.float64)
    count = np.zeros(n_q, dtype=np.int32)
    for q, terms in enumerate(product(L, R)):
        cand = candidates(terms, mode, q, norm_q, norm_j, shrink, mask, None if seen is None else set(seen[q]))
        best = order(cand, mode)[:k]
        count[q] = len(best)
        for r, (j, v) in enumerate(best):
            ids[q, r], vals[q, r] = j, v + 0.0
    return ids, vals, count


def log_views(user, item, w, n_users, n_items):
    """(rows of items: [(user, w)], rows of users: [(item, w)]), each in (id of the other side, input row) order"""
    by_item = [[] for _ in range(n_items)]
    by_user = [[] for _ in range(n_users)]
    rows = sorted(range(len(user)), key=lambda r: (int(user[r]), int(item[r]), r))
    for r in rows:
        by_user[int(user[r])].append((int(item[r]), float(w[r])))
    rows = sorted(range(len(user)), key=lambda r: (int(item[r]), int(user[r]), r))
    for r in rows:
        by_item[int(item[r])].append((int(user[r]), float(w[r])))
    return by_item, by_user


def similarity(user, item, w, n_users, n_items, k, shrink=0.0):
    """ItemKNN.fit: (ids, vals, count) [n_items, k]; a duplicated (user, item) row never pairs the item with itself and
    counts twice against the other items"""
    by_item, by_user = log_views(user, item, w, n_users, n_items)
    nrm = norms(item, w, n_items)
    return topk(by_item, by_user, k, FIT, nrm, nrm, shrink)


def table(ids, vals, count):
    """{i: [(j, s), ...]} of a similarity block"""
    return {i: [(int(ids[i, r]), float(vals[i, r])) for r in range(int(count[i]))] for i in range(len(count))}


def predict_terms(sim, log_user, log_item, users):
    """{u: {j: [s, ...]}}: one term per (log row (u, i), neighbour j of i); the log's relevance does not enter"""
    out = {int(u): {} for u in users}
    for u, i in zip(log_user, log_item):
        u, i = int(u), int(i)
        if u in out:
            for j, s in sim.get(i, ()):
                out[u].setdefault(j, []).append(s)
    return out


def predict(sim, log_user, log_item, users, items, k, filter_seen_items=True):
    """{u: [(j, score), ...]}: at most k rows per user by (score descending, j ascending), only j in `items`, without
    the user's own items when filter_seen_items"""
    items = set(int(j) for j in items)
    seen = {}
    for u, i in zip(log_user, log_item):
        seen.setdefault(int(u), set()).add(int(i))
    out = {}
    for u, terms in predict_terms(sim, log_user, log_item, users).items():
        cand = {j: math.fsum(ts) for j, ts in terms.items()
                if j in items and not (filter_seen_items and j in seen.get(u, ()))}
        out[u] = order(cand, PREDICT)[:k]
    return out


def pair_scores(sim, log_user, log_item, pairs):
    """[score or None] per (u, j): None when no history row of u has j among its neighbours"""
    terms = predict_terms(sim, log_user, log_item, set(int(u) for u, _ in pairs))
    return [math.fsum(terms[int(u)][int(j)]) if int(j) in terms[int(u)] else None for u, j in pairs]


def tolerance(kind, ref=0.0, terms=0, n_i=0, n_j=0, sum_abs=0.0):
    """Absolute bounds on |device - yardstick|.

    'weight'      4 * 2^-52 * |ref|.  The counts and the divisions that feed log1p are exact or correctly rounded on both
                  sides; the device log1p is specified to 2 ulp, the host libm to 1; one multiply follows: 2 + 1 + 1/2
                  ulp, rounded up to 4 ulp of 2^-52.
    'similarity'  (c + n_i + n_j + 8) * 2^-53 * |ref| for non-negative weights, the yardstick fed the device's weights:
                  c rounded products summed in any order (c * 2^-53 relative, all terms of one sign), two squared norms of
                  n_i and n_j rounded squares summed in any order and halved by the square root, two square roots, and
                  the multiply, add and divide of the similarity; the yardstick's own error is about 2^-53.
    'score'       t * 2^-53 * sum|terms| for a sum of t similarities in any order."""
    if kind == "weight":
        return 4.0 * 2.0 ** -52 * abs(ref)
    if kind == "similarity":
        return (terms + n_i + n_j + 8) * EPS * abs(ref)
    if kind == "score":
        return terms * EPS * sum_abs
    raise ValueError(kind)
