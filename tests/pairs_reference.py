"""NumPy restatement of the candidate-list ranking (cqlrec_pairs_topk, include/cqlrec.h a12).

* gather_dot: the score of a (state vector, item) pair with the kernel's operation order, in float32.  A product of two
  bf16 values has at most 16 significant bits and is exact in float32, so `s = s + h * e` in float32 rounds once per
  step exactly like the kernel's fmaf; then the xor butterfly over the d/8 lanes and `+ b`.  Same bits.
* rank_lists: per row the k best admissible pairs by (score desc, item id asc) through a stable sort; a candidate listed
  twice stays twice.
* the seen anti-join: a pair whose item is in the row's seen list is not admissible."""
import numpy as np


def bf16_bits_to_f32(bits):
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def gather_dot(h_bits, e_bits, b, pair_row, pair_item):
    """h_bits [n, d] / e_bits [N, d] uint16 bf16 patterns, b [N] float32; pair p scores h[pair_row[p]] against item
    pair_item[p].  Returns float32 [n_pairs] with cqlrec_gather_dot's bits."""
    h = bf16_bits_to_f32(h_bits)[np.asarray(pair_row, np.int64)]
    e = bf16_bits_to_f32(e_bits)[np.asarray(pair_item, np.int64)]
    n, d = h.shape
    lpr = d // 8
    h, e = h.reshape(n, lpr, 8), e.reshape(n, lpr, 8)
    s = np.zeros((n, lpr), np.float32)
    for j in range(8):                       # eight sequential steps per lane
        s = (s + (h[:, :, j] * e[:, :, j]).astype(np.float32)).astype(np.float32)
    off = 1
    lanes = np.arange(lpr)
    while off < lpr:                         # s += shfl_xor(s, off), all lanes at once
        s = (s + s[:, lanes ^ off]).astype(np.float32)
        off <<= 1
    return (s[:, 0] + np.asarray(b, np.float32)[np.asarray(pair_item, np.int64)]).astype(np.float32)


def admissible(items, seen):
    """the anti-join: mask of the candidates that are not in `seen`"""
    return ~np.isin(np.asarray(items), np.asarray(seen))


def rank_list(items, scores, k, seen=None):
    """(item ids, scores) of the k best admissible candidates of ONE list, (score desc, item id asc), duplicates kept"""
    items, scores = np.asarray(items), np.asarray(scores, np.float32)
    if seen is not None and len(seen):
        m = admissible(items, seen)
        items, scores = items[m], scores[m]
    o = np.argsort(items, kind="stable")
    o = o[np.argsort(-scores[o].astype(np.float64), kind="stable")][:k]
    return items[o], scores[o]


def rank_lists(pair_off, pair_items, scores, rows, k, seen_off=None, seen_items=None):
    """the [n, k] block: idx int32 (-1 padded), val float32 (-inf padded), cnt int32.  scores is in CSR order."""
    n = len(rows)
    idx = np.full((n, k), -1, np.int32)
    val = np.full((n, k), -np.inf, np.float32)
    cnt = np.zeros(n, np.int32)
    for i, r in enumerate(rows):
        lo, hi = int(pair_off[r]), int(pair_off[r + 1])
        seen = None if seen_off is None else seen_items[int(seen_off[r]): int(seen_off[r + 1])]
        it, sc = rank_list(pair_items[lo:hi], scores[lo:hi], k, seen)
        cnt[i] = len(it)
        idx[i, :len(it)] = it
        val[i, :len(it)] = sc
    return idx, val, cnt


def csr_of_lists(lists, n_rows=None):
    """{row: list of items} (or a list of lists) -> (off int64 [n_rows + 1], items int32), each list sorted ascending"""
    if not isinstance(lists, dict):
        lists = dict(enumerate(lists))
    n_rows = (max(lists) + 1 if lists else 0) if n_rows is None else n_rows
    off = np.zeros(n_rows + 1, np.int64)
    parts = []
    for r in range(n_rows):
        it = np.sort(np.asarray(lists.get(r, []), np.int32), kind="stable")
        off[r + 1] = off[r] + len(it)
        parts.append(it)
    return off, (np.concatenate(parts) if parts else np.zeros(0, np.int32)).astype(np.int32)
