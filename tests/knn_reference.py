"""Restatement of get_nearest_items' semantics in NumPy, written from the formulas (not from the reference's text).

The reference implements them as Spark column expressions and UDFs over a cross join (replay/models/base_rec.py:
955-1030, :893-926; replay/utils.py:131, :677-697); pyspark is absent here, so the reference itself cannot serve as an
executable oracle and this file is the checker.  `dtype=np.float64` gives the mathematical answer to compare against
under an error bound; `dtype=np.float32` performs the normative fp32 operation order on tables whose sums are exact,
where the device must agree bit for bit.

    dot_product             dot(i,j)
    cosine_similarity       dot / (sqrt(n_i) * sqrt(n_j)),  n = dot(j,j);  a pair with a zero denominator is left out
    euclidean_distance_sim  1 / (1 + sqrt(max((n_i + n_j) - 2*dot, 0)))
    never j == i;  order per query: value descending, then neighbour id DESCENDING;  at most k rows per query."""
import numpy as np

METRICS = ("dot_product", "cosine_similarity", "euclidean_distance_sim")


def pair_values(V, query_ids, cand_ids, metric, dtype=np.float64):
    """(values [Q x C], admissible [Q x C]) for table V [N x d] (the bf16 values, held exactly in any float type)."""
    V = np.asarray(V).astype(dtype)
    q, c = np.asarray(query_ids, dtype=np.int64), np.asarray(cand_ids, dtype=np.int64)
    n = (V * V).sum(axis=1, dtype=dtype)
    dot = V[q] @ V[c].T
    ok = q[:, None] != c[None, :]
    if metric == "dot_product":
        return dot, ok
    if metric == "cosine_similarity":
        den = np.sqrt(n[q])[:, None] * np.sqrt(n[c])[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            return dot / den, ok & (den != 0)
    if metric == "euclidean_distance_sim":
        x = (n[q][:, None] + n[c][None, :]) - 2 * dot
        return 1 / (1 + np.sqrt(np.maximum(x, 0))), ok
    raise NotImplementedError(f"{metric} metric is not implemented, valid metrics are {', '.join(METRICS)}")


def nearest_items(V, query_ids, cand_ids, k, metric, dtype=np.float64):
    """(idx int64 [Q x k] padded with -1, val [Q x k] padded with -inf, cnt [Q])."""
    val, ok = pair_values(V, query_ids, cand_ids, metric, dtype)
    c = np.asarray(cand_ids, dtype=np.int64)
    Q = val.shape[0]
    idx, out, cnt = np.full((Q, k), -1, np.int64), np.full((Q, k), -np.inf, val.dtype), np.zeros(Q, np.int64)
    for r in range(Q):
        ids, v = c[ok[r]], val[r][ok[r]]
        if len(v) > 4 * k:                      # everything at or above the k-th value (ties included) is enough
            keep = v >= np.partition(v, len(v) - k)[len(v) - k]
            ids, v = ids[keep], v[keep]
        order = np.lexsort((-ids, -v))[:k]      # value desc, then id desc
        cnt[r] = len(order)
        idx[r, :len(order)], out[r, :len(order)] = ids[order], v[order]
    return idx, out, cnt
