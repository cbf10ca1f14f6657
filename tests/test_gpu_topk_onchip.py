"""The one-pass d = 128 top-K family of cqlrec_score_topk (item_ids = NULL, k <= 16, the whole catalogue: qtopk2_kernel in
csrc/qhead_topk2.hip, qtopk4_kernel in csrc/qhead_topk4.hip, then topk_merge_kernel), THROUGH THE C ABI, on non-dyadic
inputs against the float64 certificate of helpers.topk_certificate, plus bitwise self-consistency: prefix over k (across
the KC = 10 | 16 instantiations), qtopk4 against qtopk2 on the same users, the two phases against the single call.

Which kernel a (n_users, n_cand, k) reaches -- helpers.tk2_geometry restates it, test_case_table_reaches_both_kernels
asserts the tables below against it with the device's CU count:
    kernel  qtopk4_kernel<128, lists?, KC> (512 users per block) when n_users >= 512 * 160 = 81 920, else
            qtopk2_kernel<128, KC> (256 users per block);  KC = 10 (k <= 10) | 16 (k = 11..16)
    slices  want = min(ceil(CUs / user blocks), stages / 8, 16), at least 1, with stages = ceil(n_cand / 64);
            a slice holds ceil(stages / want) stages;  nsplit = ceil(n_cand / slice)
    seen    qtopk2: dense bitmap.  qtopk4: entry lists (with an overflow area) built in the bitmap's space, or -- picked
            on the device when they do not fit -- the bitmap; cqlrec_topk_seen_form tells which (0 lists, 1 bitmap).
            Without seen rows: a single launch without a guard word; no seen phase writes the word the function reads,
            so it is not asked (TopkDevice.run gives -1)

A. qtopk2_kernel.  k runs along the chain 1, 5, 10, 11, 16 (both KC) unless stated; nsplit at 256 CUs.

    case     users  n_cand  kind      seen  nsplit  what it is for
    p_5003     300    5 003  plain     rows    9     2 user blocks, the second partial; last stage holds 11 items
    n_40k      257   40 000  neg       rows   16     16 slices, the last one shorter; every score negative (key order)
    s_5003     300    5 003  straddle  rows    9     the k-th score changes sign across users
    w_40k       64   40 000  wide      rows   16     one block, a quarter full
    r_5003     300    5 003  ramp      rows    9     queue / merge pressure in every stage
    d_5003     300    5 003  down      rows    9     bound fixed in stage 0; every later slice hands in lists that lose
    p_100      255      100  plain     rows    1     one slice, N < 128, two stages
    p_64        33       64  plain     -       1     exactly one stage
    p_65        33       65  plain     -       1     one stage plus one item
    p_5         33        5  plain     rows    1     n_cand < k at k = 10, 11, 16: padding -1 / -inf, cnt = admissible
    p_1          1        1  plain     -       1     one user, one candidate
    f1, f3      70    5 003  flat1/3   rows    9     ties everywhere, seen rows on top; bit-identical to O.topk_rows
    y_5003     300    5 003  dyadic    rows    9     bit-identical to O.topk_rows, k = 10, 16

"rows" is helpers._seen_rows: a CSR with more rows than users reached through a non-monotone seen_rows map in which
users 1 and 2 share a row; row lengths 0, 1, 511, 512, 513 and 3 000; half of every row the user's best items, the rest
random ids, some past the catalogue; user 8 has seen its best n_cand - 40 items, user 9 all but 5, user 10 all.

B. qtopk4_kernel: 512 * 160 + 300 = 82 220 users, generated independently (the smallest launch the default dispatch
gives it; the last block is partial, its third wave partly filled).  The device sees everybody; the certificate and the
oracle run on ~730 checked users `us` (0..3, 127, 128, 511, 512, 65 535, 65 536, the last 302, 400 random ones and the
crafted ones).  Every user's seen row is reached through a non-monotone map with shared rows; the crafted rows of A sit
at users base + 0..10 for base = 0, 512 * 77 + 256 and 512 * 160 + 256: three different waves, the last one the partly
filled wave of the partial block (topk_onchip_cases.build_q4_case).

    case        n_cand  kind      seen load                                              k       nsplit  seen form
    q4_light     5 003  plain     0..7 random ids + some of the best items               10, 16    2     lists
    q4_ramp      5 003  ramp      light                                                  10, 16    2     lists
    q4_neg_1s      700  neg       light                                                   5, 11    1     lists (11 stages, the last of 60 items)
    q4_popular   5 003  straddle  light + 3 items seen by 97 %, two of them in one       10, 16    2     lists, overflow area
                                  stage; the ids of CSR rows < 300 repeated
    q4_heavy       700  wide      light + a random half of the catalogue per user        10, 16    1     bitmap (lists do not fit)
    q4_noseen    5 003  plain     none                                                    1, 16    2     - (no guard word)
    q4_flat3       700  flat3     light                                                  10, 16    1     lists; bit-identical to the oracle

Per case: sentinel-filled outputs and a poisoned guard behind the declared workspace; certificate with all five checks and
no excluded rows (flat, dyadic: bit-identity to O.topk_rows); share of boundary users <= 0.10 at every k; bitwise prefix
equality between consecutive k, across KC = 10 | 16 (both instantiations run the same score chain and order by
(score, row)).  B also: the first 700 users alone, on the same device operands, take qtopk2_kernel with another slicing
and must equal rows 0..699 of the big launch bit for bit (which also closes the certificate's blind spot -- a dropped
item within eps of the k-th -- for them); q4_light and q4_heavy: CQLREC_TOPK_SEEN_BESIDE + CQLREC_TOPK_SCORE on a fresh
workspace equal CQLREC_TOPK_ALL for every one of the 82 220 users.

Every case prints its largest |val - Q64| / eps and its boundary shares (run with -s).  With an exact fp32 top-k standing
in for the kernels (test_topk_onchip_cases_cpu.py) the ratio stays below 0.04 and every share below the cap."""
import copy

import numpy as np
import pytest
import torch

from replay_cql_amd import _native as N

from helpers import TopkDevice, TopkReference, _assert_prefix, _assert_same, _no_sentinel, _oracle, tk2_geometry, topk_certificate
from topk_onchip_cases import (BITMAP, CASES_A, CASES_B, D, LISTS, NO_SEEN, ORACLE_KINDS, Q4_CROSS, Q4_PHASE_CASES, Q4_USERS,
                               SHARE_CAP, build_a_case, build_q4_case, q4_crafted_admissible, q4_subset)

pytestmark = pytest.mark.gpu

GUARD = 1 << 16
TOPK_ALL, TOPK_SCORE, TOPK_SEEN_BESIDE = 0, 2, 3          # CQLREC_TOPK_* of cqlrec.h


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_case_table_reaches_both_kernels():
    """Both tables against tk2_geometry at the device's CU count: qtopk2 and qtopk4 at both KC, one slice and several for
    each kernel, 16 slices for qtopk2.  (No launch: a later change of the dispatch makes the table fail instead of
    silently moving the cases.)"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    reached, slices = set(), {"qtopk2": set(), "qtopk4": set()}
    for cid, n_users, n_cand, _, _, ks in CASES_A:
        for k in ks:
            kernel, kc, upb, nsplit, _ = tk2_geometry(n_users, n_cand, k, n_cu)
            assert (kernel, upb) == ("qtopk2", 256), cid
            reached.add((kernel, kc))
            slices[kernel].add(nsplit)
    for cid, n_cand, _, _, ks, _ in CASES_B:
        for k in ks:
            kernel, kc, upb, nsplit, _ = tk2_geometry(Q4_USERS, n_cand, k, n_cu)
            assert (kernel, upb) == ("qtopk4", 512), cid
            reached.add((kernel, kc))
            slices[kernel].add(nsplit)
            alone = tk2_geometry(Q4_CROSS, n_cand, k, n_cu)
            assert alone[0] == "qtopk2" and (alone[3] != nsplit or nsplit == 1), f"{cid}: the cross-kernel run {alone}"
    assert reached == {(kern, kc) for kern in ("qtopk2", "qtopk4") for kc in (10, 16)}
    for kernel, ns in slices.items():
        assert 1 in ns and max(ns) > 1, (kernel, ns)
    assert 16 in slices["qtopk2"]
    assert {c[5] for c in CASES_B} == {LISTS, BITMAP, NO_SEEN}
    assert tk2_geometry(512 * 160 - 1, 5003, 10, n_cu)[0] == "qtopk2" and tk2_geometry(512 * 160, 5003, 10, n_cu)[0] == "qtopk4"


def _certify(cid, res, ks, c, ref, what):
    """certificate or oracle for every k on the users of c; returns (worst ratio, shares)"""
    worst, shares = 0.0, {}
    for k in ks:
        if ref is None:
            _assert_same(res[k], _oracle(c, k), f"{cid} k={k} against the oracle{what}")
            continue
        r = topk_certificate(*res[k], c["Hb"], c["E_c"], c["b_c"], k, seen=c["seen"], seen_rows=c["rows"], ref=ref)
        worst, shares[k] = max(worst, r["ratio"]), r["share"]
        assert r["share"] <= SHARE_CAP, (cid, k, r)
    return worst, shares


@pytest.mark.parametrize("case", CASES_A, ids=[c[0] for c in CASES_A])
def test_qtopk2(lib, case):
    """One row of table A: every k of its chain through cqlrec_score_topk with item_ids = NULL."""
    cid, n_users, n_cand, kind, with_seen, ks = case
    c = build_a_case(case)
    dev = TopkDevice(lib, c["Hb"], c["E_c"], c["b_c"], seen=c["seen"], seen_rows=c["rows"])
    ref = None if kind in ORACLE_KINDS else TopkReference(c["Hb"], c["E_c"], c["b_c"])
    res = {}
    for k in ks:
        res[k] = dev.run(k, use_ids=False, guard_bytes=GUARD)
        _no_sentinel(res[k], f"{cid} k={k}")
    worst, shares = _certify(cid, res, ks, c, ref, "")
    for k2, k1 in zip(ks[:-1], ks[1:]):
        _assert_prefix(res[k2], res[k1], k2, f"{cid}: k={k2} against the first columns of k={k1} (boundary shares {shares})")
    if kind == "straddle":
        kth = res[16][1][:, 15][res[16][2] == 16]
        assert (kth > 0).any() and (kth < 0).any(), "the 16-th best score does not change sign across users"
    if kind == "neg":
        for k in ks:
            assert np.all(res[k][1][res[k][0] >= 0] < 0)
    if with_seen and n_users > 10 and n_cand >= 3000:
        adm = (~c["mask"]).sum(1)                 # the case is what the docstring says (the random ids may hit a few more)
        assert adm[10] == 0 and 0 < adm[9] <= 5 and 25 <= adm[8] <= 40, adm[8:11]
        assert np.array_equal(res[ks[-1]][2][8:11], np.minimum(adm[8:11], ks[-1]))
    if n_cand < ks[-1]:
        adm = np.full(n_users, n_cand) if c["mask"] is None else (~c["mask"]).sum(1)
        assert np.array_equal(res[ks[-1]][2], np.minimum(adm, ks[-1]))
    print(f"\n[on-chip] {cid}: max |val - Q64| / eps = {worst:.4f}; boundary shares {shares}")


@pytest.mark.parametrize("case", CASES_B, ids=[c[0] for c in CASES_B])
def test_qtopk4(lib, case):
    """One row of table B: both k on all 82 220 users; certificate / oracle on the checked users; the seen form; the first
    700 users again through qtopk2_kernel; (q4_light, q4_heavy) the two phases against the single call."""
    cid, n_cand, kind, load, ks, form = case
    c = build_q4_case(cid, n_cand, kind, load)
    us, sub = c["us"], q4_subset(c)
    dev = TopkDevice(lib, c["Hb"], c["E_c"], c["b_c"], seen=c["seen"], seen_rows=c["rows"])
    ref = None if kind in ORACLE_KINDS else TopkReference(sub["Hb"], sub["E_c"], sub["b_c"])
    res, checked = {}, {}
    for k in ks:
        res[k] = dev.run(k, use_ids=False, guard_bytes=GUARD, query_form=True)
        assert dev.seen_form == form, f"{cid} k={k}: seen form {dev.seen_form} (0 lists, 1 bitmap, -1 none), expected {form}"
        _no_sentinel(res[k], f"{cid} k={k}")
        checked[k] = tuple(a[us] for a in res[k])
    worst, shares = _certify(cid, checked, ks, sub, ref, " (row j = user us[j])")
    _assert_prefix(res[ks[0]], res[ks[1]], ks[0], f"{cid}: k={ks[0]} against the first columns of k={ks[1]} (shares {shares})")
    if kind == "straddle":
        kth = res[16][1][:, 15][res[16][2] == 16]
        assert (kth > 0).any() and (kth < 0).any(), "the 16-th best score does not change sign across users"
    if kind == "neg":
        for k in ks:
            assert np.all(res[k][1][res[k][0] >= 0] < 0)
    if load != "none":
        adm = q4_crafted_admissible(c)
        assert np.all(adm[:, 2] == 0) and np.all((0 < adm[:, 1]) & (adm[:, 1] <= 5)) and \
            np.all((25 <= adm[:, 0]) & (adm[:, 0] <= 40)), adm
        pos = np.searchsorted(us, c["crafted"])
        want = np.minimum((~c["mask"]).sum(1)[pos], ks[-1])
        assert np.array_equal(res[ks[-1]][2][c["crafted"]], want)
    # ---- the first 700 users alone: qtopk2_kernel, another slicing, the same device operands
    if kind not in ("flat1", "flat3"):
        small = copy.copy(dev)
        small.n_users, small.H = Q4_CROSS, dev.H[:Q4_CROSS]
        small.rows = None if dev.rows is None else dev.rows[:Q4_CROSS]
        for k in ks:
            alone = small.run(k, use_ids=False, guard_bytes=GUARD)
            _no_sentinel(alone, f"{cid} k={k}, the first {Q4_CROSS} users alone")
            _assert_same(alone, tuple(a[:Q4_CROSS] for a in res[k]),
                         f"{cid} k={k}: the first {Q4_CROSS} users alone (qtopk2_kernel) against the launch of all (qtopk4_kernel)")
    # ---- the seen phase beside, then the scoring phase, on a fresh workspace
    if cid in Q4_PHASE_CASES:
        for k in ks:
            two = dev.run(k, use_ids=False, guard_bytes=GUARD, phases=(TOPK_SEEN_BESIDE, TOPK_SCORE), query_form=True)
            assert dev.seen_form == form
            _assert_same(two, res[k], f"{cid} k={k}: CQLREC_TOPK_SEEN_BESIDE + CQLREC_TOPK_SCORE against CQLREC_TOPK_ALL")
    print(f"\n[on-chip] {cid}: max |val - Q64| / eps = {worst:.4f}; boundary shares {shares}")
