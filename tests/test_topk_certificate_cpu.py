"""CPU self-test of the top-K certificate (helpers.topk_certificate): what justifies that its only slack is eps.

The "kernel" is an exact NumPy top-k over fp32 scores.  Scores summed in fp32 in three different orders (16-wide chunks
with the bias first, as the MFMA chains do; strictly sequential with the bias last; BLAS) must be ACCEPTED -- values and
selection both taken from the fp32 scores -- with and without seen rows, with a candidate subset, with fewer than k
admissible items.  Each fault a top-K kernel could make must be REJECTED on its own, under the check that names it."""
import functools

import numpy as np
import pytest

from helpers import TOPK_KINDS, TopkReference, _np_topk, topk_certificate, topk_inputs

N_USERS, N_CAT, K = 24, 24000, 10
DS = (64, 128, 256)


def _scores(Hb, Ec, bc, order):
    if order == "blas":
        return (Hb @ Ec.T + bc).astype(np.float32)
    d = Hb.shape[1]
    if order == "chunk16":                    # bias first, then one fp32 partial per 16 columns
        acc = np.broadcast_to(bc, (Hb.shape[0], Ec.shape[0])).astype(np.float32)
        for s in range(0, d, 16):
            acc = (acc + (Hb[:, s:s + 16] @ Ec[:, s:s + 16].T).astype(np.float32)).astype(np.float32)
        return acc
    acc = np.zeros((Hb.shape[0], Ec.shape[0]), np.float32)     # strictly sequential, bias last
    for i in range(d):
        acc += Hb[:, i:i + 1] * Ec[None, :, i]
    return (acc + bc).astype(np.float32)


@functools.lru_cache(maxsize=2)
def _case(d, kind):
    """A candidate subset of the catalogue, seen rows reached through a non-monotone map (users 1 and 2 share one), half of
    every row the user's best items, some seen ids that are no candidates, user 3 left with 4 admissible items, user 4
    with none."""
    Hb, Eb, b = topk_inputs(kind, N_USERS, N_CAT, d, 100 + d, k_ref=K)
    rng = np.random.default_rng(d)
    ids = np.sort(rng.choice(N_CAT, 20011, replace=False)).astype(np.int64)
    Ec, bc = Eb[ids], b[ids]
    S = _scores(Hb, Ec, bc, "blas")
    n_rows = N_USERS + 5
    rows_of = rng.permutation(n_rows)[:N_USERS]
    rows_of[2] = rows_of[1]
    lens = rng.integers(0, 60, N_USERS)
    lens[0] = 0
    rows = [np.sort(rng.choice(N_CAT, 7, replace=False)) for _ in range(n_rows)]
    for u in range(N_USERS):
        if u == 2:
            continue
        best = ids[np.argsort(-S[u], kind="stable")]
        n_best = len(ids) - 4 if u == 3 else (len(ids) if u == 4 else lens[u] // 2)
        rows[rows_of[u]] = np.unique(np.concatenate([best[:n_best], rng.integers(0, N_CAT, lens[u] - lens[u] // 2)]))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    items = np.concatenate(rows).astype(np.int32)
    mask = np.zeros(S.shape, bool)
    for u in range(N_USERS):
        mask[u] = np.isin(ids, rows[rows_of[u]])
    ref = TopkReference(Hb, Ec, bc)
    return dict(Hb=Hb, Ec=Ec, bc=bc, ids=ids, seen=(off, items), rows=rows_of.astype(np.int32), mask=mask, ref=ref, S=S)


def _cert(c, idx, val, cnt, k=K, subset=True, seen=True):
    return topk_certificate(idx, val, cnt, c["Hb"], c["Ec"], c["bc"], k, ids=c["ids"] if subset else None,
                            seen=c["seen"] if seen else None, seen_rows=c["rows"] if seen else None, ref=c["ref"])


@pytest.mark.parametrize("kind", TOPK_KINDS)
@pytest.mark.parametrize("d", DS)
def test_every_fp32_order_is_accepted(d, kind):
    c = _case(d, kind)
    worst = 0.0
    for order in ("chunk16", "seq", "blas"):
        S = _scores(c["Hb"], c["Ec"], c["bc"], order)
        for k in (K, 100):
            r = _cert(c, *_np_topk(S, k, c["ids"], c["mask"]), k=k)                       # subset + seen rows, short lists
            worst = max(worst, r["ratio"])
            if k <= 16:
                assert r["share"] <= 0.25, r
        r = _cert(c, *_np_topk(S, K, c["ids"]), seen=False)                               # subset, nothing seen
        worst = max(worst, r["ratio"])
        pos = np.arange(len(c["ids"]))
        r = _cert(c, *_np_topk(S, K, pos), subset=False, seen=False)                      # ids = candidate rows
        worst = max(worst, r["ratio"])
    assert worst < 0.25, worst          # any fp32 order stays far inside the worst-case bound (measured: <= 0.06)
    # fewer candidates than k
    sub = slice(0, 7)
    r7 = topk_certificate(*_np_topk(c["S"][:, sub], K, c["ids"][sub]), c["Hb"], c["Ec"][sub], c["bc"][sub], K, ids=c["ids"][sub])
    assert r7["share"] == 0.0


def _good(c):
    return tuple(a.copy() for a in _np_topk(c["S"], K, c["ids"], c["mask"]))


def _reject(c, idx, val, cnt, what):
    with pytest.raises(AssertionError, match=what):
        _cert(c, idx, val, cnt)


@pytest.mark.parametrize("kind", TOPK_KINDS)
@pytest.mark.parametrize("d", DS)
def test_every_fault_is_rejected(d, kind):
    c = _case(d, kind)
    ids, S, mask = c["ids"], c["S"], c["mask"]
    _cert(c, *_good(c))
    (lo, hi, Q, A), = list(c["ref"].blocks())
    Sm = np.where(mask, -np.inf, S)
    order = np.argsort(-Sm, axis=1, kind="stable")

    # the k-th item replaced by the (k+1)-th, for a user whose gap exceeds 2 eps
    gap_ok = [u for u in range(5, N_USERS)
              if Q[u, order[u, K - 1]] - Q[u, order[u, K]] > 1.01 * (A[u, order[u, K - 1]] + A[u, order[u, K]])]
    assert gap_ok, "no user with a clear gap: choose another seed"
    u = gap_ok[0]
    idx, val, cnt = _good(c)
    idx[u, K - 1], val[u, K - 1] = ids[order[u, K]], Sm[u, order[u, K]]
    _reject(c, idx, val, cnt, r"\(5\) better items left out for 1 users; worst: user %d \[c %d " % (u, order[u, K - 1]))

    # a whole 32-item group with the best item dropped; a 64-item (tg = 2) group dropped
    for width in (32, 64):
        u = 7
        g = order[u, 0] // width
        drop = mask.copy()
        drop[u, g * width:(g + 1) * width] = True
        _reject(c, *_np_topk(S, K, ids, drop), r"\(5\) better items left out for 1 users; worst: user 7 \[c %d /32:%d " %
                (order[u, 0], order[u, 0] // 32))

    # two adjacent entries swapped
    idx, val, cnt = _good(c)
    assert val[9, 3] != val[9, 4]
    idx[9, [3, 4]], val[9, [3, 4]] = idx[9, [4, 3]], val[9, [4, 3]]
    _reject(c, idx, val, cnt, r"\(4\) values ascend: user 9 at rank 3/4")

    # a seen item returned (with its true score)
    idx, val, cnt = _good(c)
    p = int(np.nonzero(mask[10])[0][0])
    idx[10, 0], val[10, 0] = ids[p], max(S[10, p], val[10, 1])
    _reject(c, idx, val, cnt, r"\(2\) seen items returned: user 10 \[c %d " % p)

    # an id outside the candidate set
    idx, val, cnt = _good(c)
    idx[11, 2] = np.setdiff1d(np.arange(N_CAT), ids)[5]
    _reject(c, idx, val, cnt, r"\(2\) user 11: ids outside the candidate set")

    # a duplicated id
    idx, val, cnt = _good(c)
    idx[12, 5], val[12, 5] = idx[12, 4], val[12, 4]
    _reject(c, idx, val, cnt, r"\(2\) duplicated: user 12")

    # cnt off by one, both ways
    for delta in (-1, 1):
        idx, val, cnt = _good(c)
        cnt[3 if delta > 0 else 13] += delta
        _reject(c, idx, val, cnt, r"\(1\) count")

    # a value off by 2 eps
    idx, val, cnt = _good(c)
    q, e = Q[14, order[14, 0]], A[14, order[14, 0]]
    val[14, 0] = np.float32(q + 2.0 * e + abs(q) * 2.0 ** -23)
    _reject(c, idx, val, cnt, r"\(3\) values off by more than eps for 1 users; worst: user 14 \[c %d " % order[14, 0])

    # a valid id in the padding (user 3 has 4 admissible items)
    idx, val, cnt = _good(c)
    assert cnt[3] == 4
    idx[3, 6] = ids[order[5, 0]]
    _reject(c, idx, val, cnt, r"\(2\) padding is not -1 / -inf: users \[3\]")
    idx, val, cnt = _good(c)
    val[3, 9] = np.float32(-1e30)
    _reject(c, idx, val, cnt, r"\(2\) padding")

    # values taken from the wrong user's row
    idx, val, cnt = _good(c)
    val[15] = val[16]
    _reject(c, idx, val, cnt, r"\(3\) values off")


def test_equal_values_must_come_in_ascending_id_order():
    """duplicate catalogue rows: items 2c and 2c + 1 score the same to the bit"""
    Hb, Eb, b = topk_inputs("plain", 8, 4000, 64, 5)
    Eb[1::2], b[1::2] = Eb[0::2], b[0::2]
    S = _scores(Hb, Eb, b, "blas")
    ids = np.arange(4000)
    idx, val, cnt = _np_topk(S, K, ids)
    assert np.all(val[:, 0] == val[:, 1]) and np.all(idx[:, 0] + 1 == idx[:, 1])
    topk_certificate(idx, val, cnt, Hb, Eb, b, K)
    assert topk_certificate(*_np_topk(S, 9, ids), Hb, Eb, b, 9)["share"] == 1.0      # ranks 9 / 10 are such a pair
    idx[5, [0, 1]] = idx[5, [1, 0]]
    with pytest.raises(AssertionError, match=r"\(4\) equal values, ids not ascending: user 5 at rank 0/1"):
        topk_certificate(idx, val, cnt, Hb, Eb, b, K)
    # -0.0 and +0.0 are equal values: the ids decide
    val[:] = np.float32(0.0)
    val[:, 1::2] = np.float32(-0.0)
    Hz = np.zeros_like(Hb)
    bz = np.zeros_like(b)
    idx[:] = np.arange(K)
    topk_certificate(idx, val, cnt, Hz, Eb, bz, K)
    idx[2, [6, 7]] = idx[2, [7, 6]]
    with pytest.raises(AssertionError, match=r"\(4\) equal values"):
        topk_certificate(idx, val, cnt, Hz, Eb, bz, K)


def test_chunked_reference_equals_the_cached_one(monkeypatch):
    """the sweep over several item chunks (catalogues beyond 64 x 262 144 / n_users) gives the same verdicts"""
    import helpers
    c = _case(64, "plain")
    whole = _cert(c, *_good(c))
    monkeypatch.setattr(helpers, "TOPK_CERT_BLOCK", N_USERS * 3001)
    ref = TopkReference(c["Hb"], c["Ec"], c["bc"])
    assert ref.step == 3001
    parts = topk_certificate(*_good(c), c["Hb"], c["Ec"], c["bc"], K, ids=c["ids"], seen=c["seen"], seen_rows=c["rows"], ref=ref)
    assert parts == whole
    assert topk_certificate(*_np_topk(c["S"], 100, c["ids"], c["mask"]), c["Hb"], c["Ec"], c["bc"], 100, ids=c["ids"],
                            seen=c["seen"], seen_rows=c["rows"], ref=ref)["ratio"] < 0.25
    idx, val, cnt = _good(c)
    u, best = 7, int(np.argmax(np.where(c["mask"][7], -np.inf, c["S"][7])))
    drop = c["mask"].copy()
    drop[u, best // 32 * 32: best // 32 * 32 + 32] = True
    with pytest.raises(AssertionError, match=r"\(5\) better items left out for 1 users; worst: user 7 \[c %d " % best):
        topk_certificate(*_np_topk(c["S"], K, c["ids"], drop), c["Hb"], c["Ec"], c["bc"], K, ids=c["ids"], seen=c["seen"],
                         seen_rows=c["rows"], ref=ref)
