"""The two-pass top-K family of cqlrec_score_topk (csrc/topk.hip: QM_TILEMAX + transpose + topk_select_small_kernel /
topk_select_kernel), THROUGH THE C ABI, on non-dyadic inputs against the float64 certificate of helpers.topk_certificate,
plus bitwise self-consistency (prefix over k, identity subset) and the layers above it (CQLCore.score_topk, CQL.predict).

The family is taken when item_ids != NULL (any k) or k > 16.  Which instantiation a (n_cand, k) reaches:
    tg = 1, doubled while ceil(ceil(n_cand / 32) / tg) > 4096;  ngroups = ceil(ceil(n_cand / 32) / tg)
    KPL = 16 (ngroups <= 1024: n_cand <= 32 768) | 32 (<= 2048: n_cand <= 65 536) | 64 (above)
    k <= 16: topk_select_small_kernel<D, KPL>;  17..512: topk_select_kernel<D, KPL, 1024>;  513..2048: <D, KPL, 4096>

    case        D    n_cand  KPL tg  ids       kind      users seen  k                                reaches
    a64_3k      64     3 000  16  1  subset    plain      300  rows  1 10 16 | 17 100 512 | 513 2048  small<64,16> select<64,16,1024|4096>
    a64_40k     64    40 000  32  1  subset    neg         32  rows  (the same chain)                 small<64,32> select<64,32,*>
    a64_100k    64   100 003  64  1  subset    wide        24  rows  (the same chain)                 small<64,64> select<64,64,*>
    a64_33      64        33  16  1  subset    straddle    24  rows  1 10 16 17 100 513 (k > n_cand)  small<64,16> select<64,16,*>
    a128_3k    128     3 000  16  1  subset    wide        32  rows  (the chain)                      small<128,16> select<128,16,*>
    a128_40k   128    40 000  32  1  subset    plain       32  rows  (the chain)                      small<128,32> select<128,32,*>
    a128_100k  128   100 003  64  1  subset    straddle    24  rows  (the chain)                      small<128,64> select<128,64,*>
    a128_140k  128   140 001  64  2  subset    neg         24  rows  10 16 17 100 513                 tg = 2 at both kernels (4 376 tiles)
    a64_140k    64   140 033  64  2  subset    plain       24  rows  16 17                            tg = 2, 4 377 tiles: the last group holds one
    a128_1     128         1  16  1  subset    plain        1  -     1 10 17 513                      one user, one candidate
    a256_3k    256     3 000  16  1  subset    neg         32  rows  (the chain)                      small<256,16> select<256,16,*>
    a256_40k   256    40 000  32  1  subset    straddle    32  rows  (the chain)                      small<256,32> select<256,32,*>
    a256_100k  256   100 003  64  1  subset    plain       24  rows  (the chain)                      small<256,64> select<256,64,*>
    a256_31    256        31  16  1  subset    wide        24  rows  1 16 17 2048                     k > n_cand, one partial tile
    b128_40k   128    40 000  32  1  subset    plain+boost 24  -     1 10 16 17                       refill() without seen items
    i64_40k     64    40 000  32  1  identity  straddle    32  rows  10 16 17 100 512 513 2048        item_ids = arange == NULL at k > 16
    i128_3k    128     3 000  16  1  identity  neg         32  rows  (the same)
    i256_40k   256    40 000  32  1  identity  wide        32  rows  (the same)
    f*                 3 000 / 40 000          flat1/flat3 24  rows  10 16 17 100 513                 bit-exact against O.topk_rows
    y64_40k     64    40 000  32  1  subset    dyadic      24  rows  10 100                           bit-exact against O.topk_rows
    y128_100k  128   100 003  64  1  subset    dyadic      24  rows  10 100
    y256_140k  256   140 001  64  2  subset    dyadic      24  rows  10 100

test_case_table_reaches_every_instantiation recomputes KPL / tg from n_cand with the arithmetic above and asserts that the
table reaches all 9 small and all 18 select instantiations and tg = 2 at both kernels: a later change of the dispatch
makes the table fail instead of silently moving the cases.

"rows" (see _seen_rows): a CSR with more rows than users, reached through a non-monotone seen_rows map in which users 1
and 2 share a row; row lengths 0, 1, 511, 512, 513 (around TK_SEEN_LDS = 512: longer rows are searched in global memory)
and 3 000; half of every row the user's best candidates, the rest random catalogue ids, among them ids that are no
candidates; user 8 has seen its best n_cand - 40 candidates (the selection walks nearly every group: refill() and the
TKS_CB overflow of the small kernel), user 9 all but 5 (fewer than k left), user 10 all of them.

Blind spot of the certificate: a dropped item whose float64 score is within 2 eps of the k-th.  At k <= 16 the share of
users in that position is asserted <= 0.25; at k > 16 rank k is interior to the next longer list of the chain, with
which the shorter one must agree bit for bit.  Only the boundary of the largest k of a chain (2 048, or the number of
admissible items) is covered up to eps only.

Every case prints its largest |val - Q64| / eps and its boundary shares (run with -s); with an exact fp32 top-k standing
in for the kernels the ratio stays below 0.04 and the shares at k <= 16 below 0.21 on these inputs."""
import numpy as np
import pandas as pd
import pytest
import torch

from oracle import cql_oracle as O
from replay_cql_amd import _native as N

from helpers import (BOOST_GROUPS, DEV, TOPK_KINDS, TopkDevice, TopkReference, _assert_prefix, _assert_same, _no_sentinel,
                     _oracle, bf16_to_np, build_case, tk_geometry, topk_certificate)

pytestmark = pytest.mark.gpu

CHAIN = (1, 10, 16, 17, 100, 512, 513, 2048)
ID_KS = (10, 16, 17, 100, 512, 513, 2048)
FLAT_KS = (10, 16, 17, 100, 513)
SHARE_CAP = 0.25
GUARD = 1 << 16

#        id           D    n_cand  KPL tg ids         kind           users seen   ks
CASES = [
    ("a64_3k",      64,    3000, 16, 1, "subset",   "plain",        300, True,  CHAIN),
    ("a64_40k",     64,   40000, 32, 1, "subset",   "neg",           32, True,  CHAIN),
    ("a64_100k",    64,  100003, 64, 1, "subset",   "wide",          24, True,  CHAIN),
    ("a64_33",      64,      33, 16, 1, "subset",   "straddle",      24, True,  (1, 10, 16, 17, 100, 513)),
    ("a128_3k",    128,    3000, 16, 1, "subset",   "wide",          32, True,  CHAIN),
    ("a128_40k",   128,   40000, 32, 1, "subset",   "plain",         32, True,  CHAIN),
    ("a128_100k",  128,  100003, 64, 1, "subset",   "straddle",      24, True,  CHAIN),
    ("a128_140k",  128,  140001, 64, 2, "subset",   "neg",           24, True,  (10, 16, 17, 100, 513)),
    ("a64_140k",    64,  140033, 64, 2, "subset",   "plain",         24, True,  (16, 17)),
    ("a128_1",     128,       1, 16, 1, "subset",   "plain",          1, False, (1, 10, 17, 513)),
    ("a256_3k",    256,    3000, 16, 1, "subset",   "neg",           32, True,  CHAIN),
    ("a256_40k",   256,   40000, 32, 1, "subset",   "straddle",      32, True,  CHAIN),
    ("a256_100k",  256,  100003, 64, 1, "subset",   "plain",         24, True,  CHAIN),
    ("a256_31",    256,      31, 16, 1, "subset",   "wide",          24, True,  (1, 16, 17, 2048)),
    ("b128_40k",   128,   40000, 32, 1, "subset",   "plain+boost",   24, False, (1, 10, 16, 17)),
    ("i64_40k",     64,   40000, 32, 1, "identity", "straddle",      32, True,  ID_KS),
    ("i128_3k",    128,    3000, 16, 1, "identity", "neg",           32, True,  ID_KS),
    ("i256_40k",   256,   40000, 32, 1, "identity", "wide",          32, True,  ID_KS),
    ("f64_flat1",   64,   40000, 32, 1, "subset",   "flat1",         24, True,  FLAT_KS),
    ("f64_flat3",   64,    3000, 16, 1, "identity", "flat3",         24, True,  FLAT_KS),
    ("f128_flat1", 128,    3000, 16, 1, "identity", "flat1",         24, True,  FLAT_KS),
    ("f128_flat3", 128,   40000, 32, 1, "subset",   "flat3",         24, True,  FLAT_KS),
    ("f256_flat1", 256,    3000, 16, 1, "subset",   "flat1",         24, True,  FLAT_KS),
    ("f256_flat3", 256,    3000, 16, 1, "subset",   "flat3",         24, True,  FLAT_KS),
    ("y64_40k",     64,   40000, 32, 1, "subset",   "dyadic",        24, True,  (10, 100)),
    ("y128_100k",  128,  100003, 64, 1, "subset",   "dyadic",        24, True,  (10, 100)),
    ("y256_140k",  256,  140001, 64, 2, "subset",   "dyadic",        24, True,  (10, 100)),
]
ORACLE_KINDS = ("flat1", "flat3", "dyadic")          # exact in every summation order: bit-identical to O.topk_rows


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_case_table_reaches_every_instantiation():
    reached, tg2, tg2_odd = set(), set(), set()
    for cid, d, n_cand, kpl, tg, _, _, _, _, ks in CASES:
        for k in ks:
            kernel, kpl_is, cb, tg_is, ngroups = tk_geometry(n_cand, k)
            assert (kpl_is, tg_is) == (kpl, tg), (cid, n_cand, kpl_is, tg_is)
            assert ngroups <= 4096 and ngroups <= 64 * kpl_is
            reached.add((kernel, d, kpl_is, cb))
            if tg_is == 2:
                tg2.add(kernel)
                if ((n_cand + 31) // 32) % 2 == 1:             # odd tile count: the last group holds one tile
                    tg2_odd.add(kernel)
    want = {("small", d, kpl, 0) for d in (64, 128, 256) for kpl in (16, 32, 64)} | \
           {("select", d, kpl, cb) for d in (64, 128, 256) for kpl in (16, 32, 64) for cb in (1024, 4096)}
    assert reached == want, sorted(want - reached)
    assert tg2 == {"small", "select"} and tg2_odd == {"small", "select"}
    # the edges of the candidate buffers and of the two kernels
    assert [tk_geometry(3000, k)[:3:2] for k in (16, 17, 512, 513)] == [("small", 0), ("select", 1024), ("select", 1024),
                                                                         ("select", 4096)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_two_pass(lib, case):
    """One row of the table: every k of its chain through cqlrec_score_topk with item_ids (guard behind the workspace,
    sentinel-filled outputs); certificate (non-dyadic kinds; share of boundary users <= 0.25 at k <= 16) or bit-identity
    to O.topk_rows (flat, dyadic); bitwise prefix equality along the chain; identity cases: item_ids = arange == NULL
    at k > 16.  The boundary of the largest k of the chain is covered up to eps only."""
    cid, d, n_cand, _, _, ids_mode, kind, n_users, with_seen, ks = case
    c = build_case(cid, d, n_cand, ids_mode, kind, n_users, with_seen)
    dev = TopkDevice(lib, c["Hb"], c["E_c"], c["b_c"], ids=c["ids"], seen=c["seen"], seen_rows=c["rows"])
    ref = None if kind in ORACLE_KINDS else TopkReference(c["Hb"], c["E_c"], c["b_c"])
    res, worst, shares = {}, 0.0, {}
    for k in ks:
        res[k] = dev.run(k, guard_bytes=GUARD)
        _no_sentinel(res[k], f"{cid} k={k}")
        if ref is None:
            _assert_same(res[k], _oracle(c, k), f"{cid} k={k} against the oracle")
            continue
        r = topk_certificate(*res[k], c["Hb"], c["E_c"], c["b_c"], k, ids=c["ids"], seen=c["seen"], seen_rows=c["rows"],
                             ref=ref)
        worst, shares[k] = max(worst, r["ratio"]), r["share"]
        if k <= 16:
            assert r["share"] <= SHARE_CAP, (cid, k, r)
    for k2, k1 in zip(ks[:-1], ks[1:]):
        _assert_prefix(res[k2], res[k1], k2, f"{cid}: k={k2} against the first columns of k={k1} (boundary shares {shares})")
    if ids_mode == "identity":
        for k in ks:
            if k > 16:
                plain = dev.run(k, use_ids=False, guard_bytes=GUARD)
                _assert_same(plain, res[k], f"{cid} k={k}: item_ids = NULL against item_ids = arange")
    if kind == "straddle" and n_cand >= 3000:
        kth = res[16][1][:, 15][res[16][2] == 16]
        assert (kth > 0).any() and (kth < 0).any(), "the 16-th best score does not change sign across users"
    if kind == "neg":
        assert np.all(res[ks[0]][1][res[ks[0]][0] >= 0] < 0)
    if kind == "plain+boost":           # the six boosted items lead every list, in id order where the scores tie
        top6 = set(c["ids"][[g * 32 + 3 for g in BOOST_GROUPS]].tolist())
        assert all(set(row[:6].tolist()) == top6 for row in res[10][0])
    if with_seen and n_users > 10 and n_cand >= 3000:
        adm = (~c["mask"]).sum(1)                 # the case is what the docstring says (the random ids may hit a few more)
        assert adm[10] == 0 and 0 < adm[9] <= 5 and 25 <= adm[8] <= 40, adm[8:11]
        assert np.array_equal(res[ks[-1]][2][8:11], np.minimum(adm[8:11], ks[-1]))
    print(f"\n[two-pass] {cid}: max |val - Q64| / eps = {worst:.4f}; boundary shares {shares}")


@pytest.mark.parametrize("kind", TOPK_KINDS)
@pytest.mark.parametrize("k", [10, 16])
@pytest.mark.parametrize("d", [64, 256])
def test_fused_family_certificate(lib, d, k, kind):
    """The fused-lists family (item_ids = NULL, k <= 16, d = 64 / 256: QM_TOPK10 at k = 10, QM_TOPK at k = 16) on a whole
    catalogue of 40 000 with seen rows: the certificate.  Nothing in the interface promises that it equals the two-pass form
    (item_ids = arange) bit for bit, but both start the same MFMA chain from the bias and order by (score, candidate row),
    so it is asserted here; a pair of forms found to differ would be a note for DESIGN.md 3.2, not a wrong answer."""
    cid = f"fused_{d}_{kind}"
    c = build_case(cid, d, 40000, "identity", kind, 32, True)
    dev = TopkDevice(lib, c["Hb"], c["E_c"], c["b_c"], ids=c["ids"], seen=c["seen"], seen_rows=c["rows"])
    fused = dev.run(k, use_ids=False, guard_bytes=GUARD)
    _no_sentinel(fused, cid)
    r = topk_certificate(*fused, c["Hb"], c["E_c"], c["b_c"], k, seen=c["seen"], seen_rows=c["rows"])
    assert r["share"] <= SHARE_CAP, r
    print(f"\n[fused] d={d} k={k} {kind}: max |val - Q64| / eps = {r['ratio']:.4f}, boundary share {r['share']:.3f}")
    _assert_same(fused, dev.run(k, guard_bytes=GUARD), f"{cid} k={k}: fused lists against the two-pass form")


# ------------------------------------------------------------------------------------------------- the layers above
def _core(n_items, d=128, n_users=150, steps=3):
    from replay_cql_amd.core import CQLCore, CQLHyper
    u, i, t, r = O.synth_log(n_users, n_items, seed=4, mean_len=14, max_len=45)
    off, items, rew = O.build_csr(u, i, t, r, n_users)
    core = CQLCore(n_items, CQLHyper(d=d, window=8, batch=128, seed=5), device=DEV)
    core.set_log(off, items, rew)
    core.train(steps)
    users = torch.arange(n_users, dtype=torch.int32, device=DEV)
    hb = core.encode(core._csr[0], core._csr[1], users)
    return core, hb


def _core_operands(core, hb, subset=None):
    Eb = bf16_to_np(core.segment(core.theta_b, "E_out"))
    b = core.segment(core.theta, "b_out").cpu().numpy()
    if subset is not None:
        Eb, b = Eb[subset], b[subset]
    return bf16_to_np(hb), Eb, b


def _host_seen(rng, n_rows, n_items, Hb, Eb, b, ids):
    """a seen CSR of n_rows rows: half of each the best candidates of the user that will use it, ascending ids"""
    S = Hb @ Eb.T + b
    rows = []
    for r in range(n_rows):
        ln = int(rng.integers(0, 60))
        best = ids[np.argsort(-S[r % S.shape[0]], kind="stable")][:ln // 2]
        rows.append(np.unique(np.concatenate([best, rng.integers(0, n_items, ln - ln // 2)])).astype(np.int32))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return off, np.concatenate(rows + [np.zeros(1, np.int32)])[:-1].astype(np.int32)


def _np3(res):
    return tuple(t.cpu().numpy() for t in res)


def test_core_score_topk_subset_seen_rows_chunked():
    """CQLCore.score_topk(cand_items = subset, seen, seen_rows, chunk) with n = 150 users in chunks of 64 (the seen_rows
    pointer is offset per chunk; the last chunk is short), on a core trained for a few steps at d = 128: certificate on
    the core's own theta_b / theta at k = 10, 100 and 512, prefix equality between them (k = 512's own boundary is covered
    up to eps only), and the chunked pass equals the one-chunk pass."""
    n_items, n = 5000, 150
    core, hb = _core(n_items, n_users=n)
    rng = np.random.default_rng(8)
    subset = np.sort(rng.choice(n_items, 3500, replace=False)).astype(np.int64)
    Hb, Ec, bc = _core_operands(core, hb, subset)
    rows_of = rng.permutation(n + 9)[:n].astype(np.int32)             # non-monotone, more CSR rows than users
    rows_of[2] = rows_of[1]
    inv = np.zeros(n + 9, np.int64)
    inv[rows_of] = np.arange(n)
    off, items = _host_seen(rng, n + 9, n_items, Hb[inv], Ec, bc, subset)
    t = lambda x, dt: torch.as_tensor(x).to(device=DEV, dtype=dt)      # noqa: E731
    kw = dict(cand_items=t(subset, torch.int64), seen=(t(off, torch.int64), t(items, torch.int32)),
              seen_rows=t(rows_of, torch.int32))
    ref = TopkReference(Hb, Ec, bc)
    res = {}
    for k in (10, 100, 512):
        res[k] = _np3(core.score_topk(hb, k, chunk=64, **kw))
        r = topk_certificate(*res[k], Hb, Ec, bc, k, ids=subset, seen=(off, items), seen_rows=rows_of, ref=ref)
        if k <= 16:
            assert r["share"] <= SHARE_CAP, r
        _assert_same(_np3(core.score_topk(hb, k, **kw)), res[k], f"k={k}: one chunk against chunks of 64")
    _assert_prefix(res[10], res[100], 10, "k=10 against k=100")
    _assert_prefix(res[100], res[512], 100, "k=100 against k=512")


def test_core_large_k_full_ranking_and_callable_states():
    """_score_topk_large_k: k = 5 000 on a 6 000-item catalogue (parts of 2 048 candidates ranked completely, merged on the
    host side of the API) with seen rows, and with a candidate subset of 4 500 (fewer than k admissible: padding).  The
    certificate runs over the complete ranking; k = 5 000 must be the prefix of the full ranking k = 6 000, whose own end
    is the end of the admissible items.  score_topk((n, fn), k > MAX_FUSED_K) used to raise AttributeError
    (the callable reached _score_topk_large_k, which reads hb.shape): it now equals the call with the vectors."""
    n_items, n = 6000, 40
    core, hb = _core(n_items, n_users=n)
    rng = np.random.default_rng(9)
    Hb, Eb, b = _core_operands(core, hb)
    allids = np.arange(n_items, dtype=np.int64)
    off, items = _host_seen(rng, n, n_items, Hb, Eb, b, allids)
    t = lambda x, dt: torch.as_tensor(x).to(device=DEV, dtype=dt)      # noqa: E731
    seen_t = (t(off, torch.int64), t(items, torch.int32))
    full = _np3(core.score_topk(hb, 6000, seen=seen_t))
    topk_certificate(*full, Hb, Eb, b, 6000, seen=(off, items))
    assert np.array_equal(full[2], n_items - np.diff(off))
    k5 = _np3(core.score_topk(hb, 5000, seen=seen_t))
    topk_certificate(*k5, Hb, Eb, b, 5000, seen=(off, items))
    _assert_prefix(k5, full, 5000, "k=5000 against the full ranking")
    subset = np.sort(rng.choice(n_items, 4500, replace=False)).astype(np.int64)
    sub = _np3(core.score_topk(hb, 5000, cand_items=t(subset, torch.int64), seen=seen_t))
    topk_certificate(*sub, Hb, Eb[subset], b[subset], 5000, ids=subset, seen=(off, items))
    assert np.all(sub[2] < 4501) and np.all(sub[0][:, 4500:] == -1)
    calls = []

    def fn(lo, hi):
        calls.append((lo, hi))
        return hb[lo:hi]
    lazy = _np3(core.score_topk((n, fn), 5000, seen=seen_t))
    assert calls == [(0, n)]
    _assert_same(lazy, k5, "callable state vectors against the vectors themselves at k = 5000")


def test_predict_on_a_log_with_id_gaps_is_certified():
    """CQL.predict on a log whose item ids have gaps: item_dim = max id + 1 exceeds the number of fit items, so `cand` stays
    a true subset and k = 10 goes through topk_select_small_kernel with item_ids and seen_rows.  The recommendations must be
    what the fitted parameters give with ids = fit items: certificate on the model's own state vectors, theta_b, theta."""
    from replay_cql_amd.cql import CQL
    u, i, t, r = O.synth_log(120, 700, seed=6, mean_len=14, max_len=40)
    i = i * 2 + i // 25                                                # injective, with gaps: most odd ids are missing
    log = pd.DataFrame({"user_idx": u, "item_idx": i.astype(np.int64), "timestamp": pd.to_datetime(t, unit="s"),
                        "relevance": r})
    m = CQL(embedding_dim=128, window=8, batch_size=64, n_steps=6, seed=3, device=DEV)
    m.fit(log)
    fit_items = np.sort(log.item_idx.unique()).astype(np.int64)
    assert m._item_dim_size > len(fit_items) + 100
    k = 10
    recs = m.predict(log, k=k)
    core = m.core
    users = np.sort(log.user_idx.unique()).astype(np.int64)
    user_ids = torch.as_tensor(users).to(DEV)
    offsets, items_d, seen = m._device_states(m._pdf_cols(log, core.device), user_ids, True)
    hb = core.encode(offsets, items_d, user_ids.to(torch.int32))
    Hb, Eb, b = _core_operands(core, hb, fit_items)
    idx = np.full((len(users), k), -1, np.int32)
    val = np.full((len(users), k), -np.inf, np.float32)
    cnt = np.zeros(len(users), np.int32)
    by_user = {uu: g for uu, g in recs.groupby("user_idx", sort=False)}
    for row, uu in enumerate(users):
        g = by_user.get(uu)
        if g is not None:
            cnt[row] = len(g)
            idx[row, :len(g)] = g.item_idx.values
            val[row, :len(g)] = g.relevance.values.astype(np.float32)
    r = topk_certificate(idx, val, cnt, Hb, Eb, b, k, ids=fit_items, seen=(offsets.cpu().numpy(), seen.cpu().numpy()),
                         seen_rows=users)
    assert r["share"] <= SHARE_CAP, r
    assert np.all(cnt == k) and set(recs.item_idx) <= set(fit_items.tolist())
