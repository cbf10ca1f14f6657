"""CPU side of the one-pass d = 128 top-K tests (test_gpu_topk_onchip.py): what justifies their share cap and shows that
the certificate still discriminates on their inputs.

An exact fp32 top-k (_np_topk over Hb Ec^T + b) stands in for the kernels.  On every non-dyadic row of both case tables,
seen rows included, the certificate must accept it at every k of the row with a boundary share <= 0.10: the reference
alone stays inside the cap, so the cap hides nothing (a row that does not gets another seed or size, never another cap).
On r_5003 and q4_popular -- scores of ~250 and of ~0 -- three faults must each be rejected under the check that names
them.  tk2_geometry is checked against hand-worked rows."""
import numpy as np
import pytest

from helpers import _np_topk, tk2_geometry, topk_certificate, topk_inputs, TopkReference
from topk_onchip_cases import (CASES_A, CASES_B, ORACLE_KINDS, Q4_BASES, Q4_CROSS, Q4_USERS, SHARE_CAP, build_a_case,
                               build_q4_case, q4_crafted_admissible, q4_subset)

A_ROWS = [c for c in CASES_A if c[3] not in ORACLE_KINDS]
B_ROWS = [c for c in CASES_B if c[2] not in ORACLE_KINDS]


def _stand_in_shares(cid, c, ks):
    ref = TopkReference(c["Hb"], c["E_c"], c["b_c"])
    worst, shares = 0.0, {}
    for k in ks:
        r = topk_certificate(*_np_topk(c["S"], k, c["ids"], c["mask"]), c["Hb"], c["E_c"], c["b_c"], k, seen=c["seen"],
                             seen_rows=c["rows"], ref=ref)
        worst, shares[k] = max(worst, r["ratio"]), r["share"]
        assert r["share"] <= SHARE_CAP, (cid, k, r)
    assert worst < 0.25, worst                    # any fp32 order stays far inside the worst-case bound
    print(f"\n[on-chip, fp32 stand-in] {cid}: max |val - Q64| / eps = {worst:.4f}; boundary shares {shares}")


@pytest.mark.parametrize("case", A_ROWS, ids=[c[0] for c in A_ROWS])
def test_reference_stays_inside_the_share_cap_a(case):
    _stand_in_shares(case[0], build_a_case(case), case[5])


@pytest.mark.parametrize("case", B_ROWS, ids=[c[0] for c in B_ROWS])
def test_reference_stays_inside_the_share_cap_b(case):
    cid, n_cand, kind, load, ks, _ = case
    c = build_q4_case(cid, n_cand, kind, load)
    _stand_in_shares(cid, q4_subset(c), ks)
    if load != "none":                            # the case is what its table says
        adm = q4_crafted_admissible(c)
        assert np.all(adm[:, 2] == 0) and np.all((0 < adm[:, 1]) & (adm[:, 1] <= 5)) and \
            np.all((25 <= adm[:, 0]) & (adm[:, 0] <= 40)), adm
        rows = c["rows"]
        assert np.any(np.diff(rows.astype(np.int64)) < 0) and np.unique(rows).size < rows.size     # non-monotone, shared rows
        assert all(rows[b + 1] == rows[b + 2] for b in Q4_BASES)
        off, items = c["seen"]
        for b in Q4_BASES:      # distinct ids per crafted row: exactly that many where the catalogue has room for them
            lens = np.array([np.unique(items[off[rows[b + o]]: off[rows[b + o] + 1]]).size for o in (0, 3, 4, 5, 6)])
            want = np.array([0, 1, 511, 512, 513])
            assert np.all(lens <= want) and np.all(lens >= (want if n_cand >= 3000 else want * 0.9)), lens
    assert Q4_BASES[0] + 10 < Q4_CROSS and Q4_BASES[2] // 512 == Q4_USERS // 512 and \
        len({(b // 512, b % 512 // 128) for b in Q4_BASES}) == 3


def test_ramp_and_down_are_what_they_say():
    """ramp: the best items are the last ones (the running k-th best rises all through the pass); down: the first ones"""
    for kind, lo, hi in (("ramp", 4700, 5003), ("down", 0, 300)):
        Hb, Eb, b = topk_inputs(kind, 50, 5003, 128, 3)
        p = topk_inputs("plain", 50, 5003, 128, 3)
        assert np.array_equal(Hb, p[0]) and np.array_equal(Eb, p[1])
        step = np.float32(0.05 if kind == "ramp" else -0.05)
        assert np.array_equal(b, p[2] + step * np.arange(5003, dtype=np.float32))
        top = np.argsort(-(Hb @ Eb.T + b), axis=1)[:, :16]
        assert top.min() >= lo and top.max() < hi


def _faults(c, k):
    """the three faults on one case (c: users x candidates, ids = candidate rows); each rejected by the check that names it"""
    ids, S, mask = c["ids"], c["S"], c["mask"]
    ref = TopkReference(c["Hb"], c["E_c"], c["b_c"])
    n_users = S.shape[0]

    def cert(idx, val, cnt):
        return topk_certificate(idx, val, cnt, c["Hb"], c["E_c"], c["b_c"], k, seen=c["seen"], seen_rows=c["rows"], ref=ref)

    def good():
        return tuple(a.copy() for a in _np_topk(S, k, ids, mask))
    cert(*good())
    (_, _, Q, A), = list(ref.blocks())
    Sm = np.where(mask, -np.inf, S)
    order = np.argsort(-Sm, axis=1, kind="stable")
    full = np.isfinite(Sm[np.arange(n_users), order[:, k]])              # more than k admissible items

    # one item dropped that is above the k-th by more than its eps: the nearest such item to the boundary, the list moves up
    found = None
    for u in np.nonzero(full)[0][11:]:
        above = [j for j in range(k) if Q[u, order[u, j]] - A[u, order[u, j]] > Sm[u, order[u, k]]]
        if above:
            found = (int(u), above[-1])
            break
    assert found, "no user with a clear gap: choose another seed"
    u, j = found
    idx, val, cnt = good()
    keep = [i for i in range(k + 1) if i != j]
    idx[u], val[u] = ids[order[u, keep]], Sm[u, order[u, keep]]
    with pytest.raises(AssertionError, match=r"\(5\) better items left out for 1 users; worst: user %d \[c %d " % (u, order[u, j])):
        cert(idx, val, cnt)
    assert j >= k - 3, "eps does not discriminate near the boundary any more"

    # a seen item returned (with its true score)
    u = int(np.nonzero(full & mask.any(1))[0][12])
    idx, val, cnt = good()
    p = int(np.nonzero(mask[u])[0][0])
    idx[u, 0], val[u, 0] = ids[p], max(S[u, p], val[u, 1])
    with pytest.raises(AssertionError, match=r"\(2\) seen items returned: user %d \[c %d " % (u, p)):
        cert(idx, val, cnt)

    # the seen row of the neighbouring user: the user's own best items, which it has seen, come back
    top = np.argsort(-S, axis=1, kind="stable")[:, :k]
    own = np.take_along_axis(mask, top, 1)
    other = np.take_along_axis(np.roll(mask, -1, axis=0), top, 1)
    u = int(np.nonzero((own & ~other).any(1)[:-1] & full[:-1])[0][5])
    wrong = mask.copy()
    wrong[u] = mask[u + 1]
    with pytest.raises(AssertionError, match=r"\(2\) seen items returned: user %d \[c " % u):
        cert(*_np_topk(S, k, ids, wrong))


def test_faults_are_rejected_on_the_ramp():
    case = next(c for c in CASES_A if c[0] == "r_5003")
    c = build_a_case(case)
    assert np.median(_np_topk(c["S"], 16, c["ids"], c["mask"])[1][:, 0]) > 200          # eps at scores of ~250
    _faults(c, 16)


def test_faults_are_rejected_with_popular_items():
    cid, n_cand, kind, load, _, _ = next(c for c in CASES_B if c[0] == "q4_popular")
    _faults(q4_subset(build_q4_case(cid, n_cand, kind, load)), 16)


def test_tk2_geometry_hand_worked():
    """at 256 CUs.  300 users: 2 blocks of 256, 128 slices wanted, 79 stages allow 79 // 8 = 9 of ceil(79 / 9) = 9 stages.
    257 x 40 000: 625 stages, capped at 16 slices of 40 stages.  82 220 users: 161 blocks of 512, ceil(256 / 161) = 2
    slices of 40 stages (5 003) or one (700: 11 stages, 11 // 8 = 1).  131 072 users: 256 blocks, one slice."""
    for k, kc in ((1, 10), (10, 10), (11, 16), (16, 16)):
        assert tk2_geometry(300, 5003, k) == ("qtopk2", kc, 256, 9, 576)
        assert tk2_geometry(257, 40000, k) == ("qtopk2", kc, 256, 16, 2560)
        assert tk2_geometry(82220, 5003, k) == ("qtopk4", kc, 512, 2, 2560)
        assert tk2_geometry(82220, 700, k)[:4] == ("qtopk4", kc, 512, 1)
        assert tk2_geometry(81919, 5003, k)[:3] == ("qtopk2", kc, 256)
        assert tk2_geometry(131072, 100000, k)[:4] == ("qtopk4", kc, 512, 1)
    assert 40000 - 15 * 2560 == 1600                                    # n_40k: the last slice is shorter
    assert tk2_geometry(300, 5003, 10, n_cu=304)[3] == 9 and tk2_geometry(82220, 5003, 10, n_cu=80)[3] == 1
    reached = {tk2_geometry(c[1], c[2], k)[:2] for c in CASES_A for k in c[5]} | \
              {tk2_geometry(Q4_USERS, c[1], k)[:2] for c in CASES_B for k in c[4]}
    assert reached == {(kern, kc) for kern in ("qtopk2", "qtopk4") for kc in (10, 16)}
