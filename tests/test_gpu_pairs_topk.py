"""Ranking of per-user candidate lists on the GPU (cqlrec_pairs_topk, include/cqlrec.h a12) through the C ABI and through
`CQL`.  No tolerance anywhere: scores are compared as bit patterns with cqlrec_gather_dot and with the float32 emulation
of tests/pairs_reference.py, selections as ids and bit patterns with the stable-sort ranking there."""

import numpy as np
import pandas as pd
import pytest
import torch

import pairs_reference as PR
from helpers import DEV, dev, keep, ptr, stream, sync, ws_bytes_tensor
from oracle import cql_oracle as O
from replay_cql_amd import _native as N
from replay_cql_amd.recommender_api import PandasRecommender

gpu = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


class Table:
    """an item table + state vectors on the device and as bf16 bit patterns on the host"""

    def __init__(self, n_items, d, n_states, seed, dyadic=False):
        rng = np.random.default_rng(seed)
        if dyadic:      # few distinct values, exact sums in any order: many pairs of a row score identically
            E = rng.integers(-1, 2, (n_items, d)).astype(np.float32) * (rng.random((n_items, 1)) < 0.5)
            E[:, 8:] = 0
            H = np.zeros((n_states, d), np.float32)
            H[:, :8] = rng.integers(0, 2, (n_states, 8))
            b = np.full(n_items, 16.0, np.float32)              # keeps every score away from +-0
        else:
            E = (rng.standard_normal((n_items, d)) * 0.3).astype(np.float32)
            H = rng.standard_normal((n_states, d)).astype(np.float32)
            b = (rng.standard_normal(n_items) * 0.1).astype(np.float32)
        self.n_items, self.d, self.b = n_items, d, b
        self.E_bits, self.H_bits = O.bf16_bits(E), O.bf16_bits(H)
        as_bf16 = lambda bits: keep(torch.as_tensor(bits.astype(np.int16)).to(DEV).view(torch.bfloat16).contiguous())  # noqa: E731
        self.E_dev, self.H_dev, self.b_dev = as_bf16(self.E_bits), as_bf16(self.H_bits), dev(b)


def run_pairs(t, off, items, rows, k, seen=None, want_score=True, ws=None):
    """one cqlrec_pairs_topk call -> (idx, val, cnt, score) as numpy (None where not asked for)"""
    lib = N.load()
    n = t.H_bits.shape[0] if rows is None else len(rows)
    nnz = len(items)
    off_d, items_d = dev(off, torch.int64), dev(np.concatenate([items, [0]]), torch.int32)
    rows_d = None if rows is None else dev(rows, torch.int32)
    s_off = s_items = None
    if seen is not None:
        s_off, s_items = dev(seen[0], torch.int64), dev(np.concatenate([seen[1], [0]]), torch.int32)
    nb = int(lib.cqlrec_pairs_topk_ws_bytes(n, nnz, t.d, k))
    assert nb > 0
    ws = ws_bytes_tensor(nb) if ws is None else ws
    keep(ws)
    score = keep(torch.full((max(nnz, 1),), float("nan"), dtype=torch.float32, device=DEV)) if want_score else None
    idx = keep(torch.full((n, max(k, 1)), -7, dtype=torch.int32, device=DEV)) if k else None
    val = keep(torch.full((n, max(k, 1)), float("nan"), dtype=torch.float32, device=DEV)) if k else None
    cnt = keep(torch.full((n,), -7, dtype=torch.int32, device=DEV)) if k else None
    N.check(lib.cqlrec_pairs_topk(ptr(t.H_dev), ptr(t.E_dev), ptr(t.b_dev), t.n_items, t.d, ptr(off_d), ptr(items_d),
                                  ptr(rows_d), n, ptr(s_off), ptr(s_items), k, ptr(ws), nb, ptr(score), ptr(idx), ptr(val),
                                  ptr(cnt), stream()), "pairs_topk")
    sync()
    np_ = lambda x: None if x is None else x.cpu().numpy()       # noqa: E731
    return np_(idx), np_(val), np_(cnt), None if score is None else score.cpu().numpy()[:nnz]


def reference(t, off, items, rows, k, seen=None):
    n_rows = len(off) - 1
    rows_ = np.arange(n_rows) if rows is None else np.asarray(rows)
    state_of_row = np.full(n_rows, -1, np.int64)
    state_of_row[rows_] = np.arange(len(rows_))
    pair_row = np.repeat(np.arange(n_rows), np.diff(off))
    sel = state_of_row[pair_row] >= 0
    score = np.full(len(items), np.nan, np.float32)
    score[sel] = PR.gather_dot(t.H_bits, t.E_bits, t.b, state_of_row[pair_row[sel]], items[sel])
    if not k:
        return None, None, None, score
    idx, val, cnt = PR.rank_lists(off, items, score, rows_, k, None if seen is None else seen[0],
                                  None if seen is None else seen[1])
    return idx, val, cnt, score


def assert_same(got, exp, k):
    gi, gv, gc, gs = got
    ei, ev, ec, es = exp
    if es is not None and gs is not None:
        assert np.array_equal(_bits(gs), _bits(es)), "score bits"
    if k:
        assert np.array_equal(gc, ec), "counts"
        assert np.array_equal(gi, ei), "item ids"
        assert np.array_equal(_bits(gv), _bits(ev)), "value bits"


def random_lists(rng, lengths, n_items):
    return PR.csr_of_lists([rng.integers(0, n_items, n) for n in lengths])


# ---- 1. bits ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", [64, 128, 256])
def test_scores_are_gather_dot_bit_for_bit(d):
    rng = np.random.default_rng(d)
    t = Table(1000, d, 37, seed=d)
    off, items = random_lists(rng, rng.integers(0, 300, 37), 1000)
    got = run_pairs(t, off, items, None, 0)
    pair_row = np.repeat(np.arange(37), np.diff(off))
    exp = PR.gather_dot(t.H_bits, t.E_bits, t.b, pair_row, items)
    assert np.array_equal(_bits(got[3]), _bits(exp))
    # cqlrec_gather_dot on the expanded inputs: what _predict_pairs computes
    lib = N.load()
    Hx = keep(t.H_dev.index_select(0, dev(pair_row, torch.int64)).contiguous())
    out = keep(torch.empty(len(items), dtype=torch.float32, device=DEV))
    N.check(lib.cqlrec_gather_dot(ptr(Hx), ptr(t.E_dev), ptr(t.b_dev), ptr(dev(items, torch.int32)), len(items), d, ptr(out),
                                  stream()), "gather_dot")
    sync()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(got[3]))
    # and with a selection beside it the scores are the same
    got10 = run_pairs(t, off, items, None, 10)
    assert np.array_equal(_bits(got10[3]), _bits(exp))


# ---- 2. selection ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1, 10, 64, 100, 512])
def test_selection_exact_over_list_lengths(k):
    rng = np.random.default_rng(k)
    lengths = [0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, 257, 5000]
    # CSR rows: every list twice with empty rows between them; the state vectors select a permuted subset
    per_row = {}
    for j, n in enumerate(lengths + lengths):
        per_row[3 * j + 1] = rng.integers(0, 1000, n)
    off, items = PR.csr_of_lists(per_row, 3 * 2 * len(lengths) + 2)
    left_out = {3 * (len(lengths) + 9) + 1, 3 * 7 + 1, 3 * 1 + 1}           # a 5000-list, a 64-list and a 1-list are not selected
    rows = rng.permutation(np.array(sorted(set(per_row) - left_out) + [0, 5]))      # two empty CSR rows among them
    t = Table(1000, 64, len(rows), seed=100 + k)
    got = run_pairs(t, off, items, rows, k)
    exp = reference(t, off, items, rows, k)
    assert_same(got, exp, k)
    assert np.isnan(exp[3]).any() and np.array_equal(np.isnan(got[3]), np.isnan(exp[3]))     # unselected rows untouched


# ---- 3. ties ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [3, 10, 64])
def test_ties_order_by_item_id_and_duplicates_stay(k):
    rng = np.random.default_rng(7 * k)
    t = Table(400, 64, 12, seed=3, dyadic=True)
    lists = [rng.integers(0, 400, n) for n in (40, 90, 200, 300, 64, 65, 5, 0, 700, 128)]
    # the same item two and three times, among them the best-scoring item of the row (so they sit at every k boundary)
    lists.append(np.concatenate([np.arange(30), [4, 4, 9, 9, 9]]))
    lists.append(np.repeat(np.arange(k // 2 + 1), 3))
    off, items = PR.csr_of_lists(lists)
    got = run_pairs(t, off, items, None, k)
    exp = reference(t, off, items, None, k)
    for i in range(12):              # the inputs do what they are for: dozens of equal scores per row
        sc = exp[3][off[i]: off[i + 1]]
        if len(sc) >= 40:
            assert np.unique(sc, return_counts=True)[1].max() >= 12
    assert_same(got, exp, k)


# ---- 4. a long row beside short ones ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_case():
    rng = np.random.default_rng(99)
    lengths = [int(x) for x in rng.integers(5, 51, 300)]
    lengths.insert(117, 70_000)
    off, items = random_lists(rng, lengths, 80_000)
    t = Table(80_000, 64, 301, seed=8)
    pair_row = np.repeat(np.arange(301), np.diff(off))
    return t, off, items, PR.gather_dot(t.H_bits, t.E_bits, t.b, pair_row, items)


@gpu
@pytest.mark.parametrize("k", [512, 10])
def test_long_row_beside_short_rows(long_case, k):
    t, off, items, score = long_case
    got = run_pairs(t, off, items, None, k)
    exp = PR.rank_lists(off, items, score, np.arange(301), k) + (score,)
    assert_same(got, exp, k)


# ---- 5. seen filter --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [5, 100])
def test_seen_filter(k):
    rng = np.random.default_rng(k)
    t = Table(1000, 128, 8, seed=31)
    cands = [np.arange(0, 60), rng.integers(0, 1000, 300), rng.integers(0, 1000, 40), np.array([7, 7, 7, 9, 12, 12]),
             rng.integers(0, 1000, 5000), np.arange(100, 130), np.zeros(0, np.int64), rng.integers(0, 1000, 64)]
    seen = [np.arange(0, 60),                      # wholly seen
            np.zeros(0, np.int64),                 # empty seen list
            np.arange(1000),                       # every item: wholly seen again, through a long seen list
            np.array([7, 500]),                    # a seen item that is listed three times among the candidates
            rng.integers(0, 1000, 400),            # a long list against a long seen list
            np.array([5, 99, 130, 999]),           # seen items absent from the candidates
            np.array([1, 2, 3]),                   # no candidates at all
            cands[7][:10]]
    seen = [np.unique(s) for s in seen]
    off, items = PR.csr_of_lists(cands)
    s_off, s_items = PR.csr_of_lists(seen)
    got = run_pairs(t, off, items, None, k, seen=(s_off, s_items))
    exp = reference(t, off, items, None, k, seen=(s_off, s_items))
    assert_same(got, exp, k)
    assert got[2][0] == 0 and got[2][2] == 0 and np.all(got[0][0] == -1) and np.all(np.isneginf(got[1][2]))
    assert got[2][3] == 3 and sorted(got[0][3][:3].tolist()) == [9, 12, 12]        # the three 7s are gone, both 12s stay
    assert not np.isnan(got[3]).any()              # out_score is complete, seen pairs included


# ---- 6. determinism --------------------------------------------------------------------------------------------------
@gpu
def test_same_call_twice_gives_the_same_bytes():
    rng = np.random.default_rng(4)
    t = Table(3000, 64, 40, seed=5)
    lengths = [int(x) for x in rng.integers(0, 200, 36)] + [9000, 13_000, 4097, 20_000]      # four rows that are cut
    off, items = random_lists(rng, rng.permutation(lengths), 3000)
    runs = []
    for fill in (0x00, 0xA5):
        nb = int(N.load().cqlrec_pairs_topk_ws_bytes(40, len(items), 64, 100))
        ws = ws_bytes_tensor(nb)
        ws.fill_(fill)                                  # whatever the workspace held before
        runs.append(run_pairs(t, off, items, None, 100, ws=ws))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    assert_same(runs[0], reference(t, off, items, None, 100), 100)


# ---- 7./8. through CQL -----------------------------------------------------------------------------------------------
def _arrow(df):
    import pyarrow as pa
    return pa.table({c: pa.array(df[c].to_numpy().astype(np.int32)) for c in ("user_idx", "item_idx")}).to_batches()


@gpu
def test_no_pairs_by_d_intermediate():
    from replay_cql_amd.cql import CQL
    U, NI, d, per = 2000, 5000, 256, 1000
    u, i, ts, r = O.synth_log(U, NI, seed=2, mean_len=8, max_len=20)
    log = pd.DataFrame({"user_idx": u, "item_idx": i, "timestamp": pd.to_datetime(ts, unit="s"), "relevance": r})
    m = CQL(embedding_dim=d, window=8, batch_size=64, n_steps=1, seed=1, device=DEV)
    m.fit(log)
    known = np.sort(log.item_idx.unique())
    rng = np.random.default_rng(0)
    users = np.sort(log.user_idx.unique())
    pairs = pd.DataFrame({"user_idx": np.repeat(users, per), "item_idx": known[rng.integers(0, len(known), len(users) * per)]})
    nnz = len(pairs)
    assert nnz >= 1_900_000
    pb, lb = _arrow(pairs), _arrow(log)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m.predict_pairs_arrow(pb, lb, k=10)
    growth = torch.cuda.max_memory_allocated() - base
    print(f"pairs {nnz}, d {d}: peak growth {growth} bytes; the expanded state block alone is {nnz * d * 2}")
    assert growth < nnz * d
    assert out.num_rows == 10 * len(users)


MU, MNI, MD, ML = 120, 700, 64, 8


@pytest.fixture(scope="module")
def fitted():
    from replay_cql_amd.cql import CQL
    u, i, ts, r = O.synth_log(MU, MNI, seed=6, mean_len=14, max_len=40)
    log = pd.DataFrame({"user_idx": u, "item_idx": i, "timestamp": pd.to_datetime(ts, unit="s"), "relevance": r})
    m = CQL(embedding_dim=MD, window=ML, batch_size=64, n_steps=12, seed=3, device=DEV)
    m.fit(log)
    rng = np.random.default_rng(12)
    known = np.sort(log.item_idx.unique())
    users = np.sort(log.user_idx.unique())
    pu = np.repeat(users[:60], 25)
    pi = known[rng.integers(0, len(known), len(pu))]
    pairs = pd.DataFrame({"user_idx": pu, "item_idx": pi})
    extra = pd.DataFrame({"user_idx": [10_000, 10_000, users[0], users[1], users[1], users[1], users[70], users[70]],
                          "item_idx": [known[0], known[1], 10**6, known[3], known[3], known[3], known[4], known[5]]})
    pairs = pd.concat([pairs, extra], ignore_index=True).sample(frac=1.0, random_state=3).reset_index(drop=True)
    sub = log[log.user_idx != users[70]]          # users[70] has pairs but no history in the passed log
    return m, log, sub, pairs, int(users[70])


@gpu
@pytest.mark.parametrize("k", [1, 3, 600])
def test_predict_pairs_k_equals_the_host_wrapper(fitted, k):
    m, _, sub, pairs, no_history = fitted
    got = m.predict_pairs(pairs, sub, k=k)
    exp = PandasRecommender._predict_pairs_wrap(m, pairs, sub, k=k)
    assert len(exp) > 0 and exp.groupby("user_idx").size().max() == min(k, 28)
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    assert np.array_equal(got.relevance.to_numpy().view(np.uint64), exp.relevance.to_numpy().view(np.uint64))
    assert 10_000 not in set(got.user_idx) and 10**6 not in set(got.item_idx)
    assert no_history in set(pairs.user_idx) and no_history not in set(got.user_idx)


@gpu
def test_predict_pairs_arrow_and_evaluate_candidates(fitted):
    from oracle import metrics_oracle as MO
    m, log, sub, pairs, no_history = fitted
    # k=None: every pair, (user, item) order, the relevance bits of predict_pairs(k=None)
    exp = m.predict_pairs(pairs, sub).sort_values(["user_idx", "item_idx"], kind="stable").reset_index(drop=True)
    got = m.predict_pairs_arrow(_arrow(pairs), _arrow(sub)).to_pandas()
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    assert np.array_equal(got.relevance.to_numpy().view(np.uint64), exp.relevance.to_numpy().view(np.uint64))
    # k: the frame of predict_pairs(k)
    got = m.predict_pairs_arrow(_arrow(pairs), _arrow(sub), k=4).to_pandas()
    pd.testing.assert_frame_equal(got, m.predict_pairs(pairs, sub, k=4), check_exact=True)
    # filter_seen_items: the anti-join with the log, with and without k
    seen = set(zip(sub.user_idx, sub.item_idx))
    pairs2 = pd.concat([pairs, sub[["user_idx", "item_idx"]].iloc[::7]], ignore_index=True)
    full = m.predict_pairs(pairs2, sub)
    unseen = full[[(u, i) not in seen for u, i in zip(full.user_idx, full.item_idx)]]
    assert len(unseen) < len(full)
    got = m.predict_pairs_arrow(_arrow(pairs2), _arrow(sub), filter_seen_items=True).to_pandas()
    exp = unseen.sort_values(["user_idx", "item_idx"], kind="stable").reset_index(drop=True)
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    got = m.predict_pairs_arrow(_arrow(pairs2), _arrow(sub), k=5, filter_seen_items=True).to_pandas()
    exp = unseen.sort_values(["user_idx", "relevance", "item_idx"], ascending=[True, False, True], kind="stable")
    exp = exp[exp.groupby("user_idx").cumcount() < 5].reset_index(drop=True)
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    with pytest.raises(ValueError, match="outside the fitted catalogue"):
        m.can_predict_cold_items = True
        try:
            m.predict_pairs_arrow(_arrow(pairs), _arrow(sub), k=2)
        finally:
            del m.can_predict_cold_items
    # evaluate_candidates == the CPU metrics on the ranked frame
    # the ground truth of a user is a SET of items (collect_set in base_metric.py:102-140); the log repeats some pairs
    test = log.sample(frac=0.1, random_state=4)[["user_idx", "item_idx"]].drop_duplicates()
    test = pd.concat([test, pd.DataFrame({"user_idx": [10_000, no_history], "item_idx": [1, 2]})], ignore_index=True)
    test = test.drop_duplicates().reset_index(drop=True)
    # held-out items among the candidates, every fourth of them listed twice; `pairs` repeats candidates of its own
    cand = pd.concat([pairs, test.iloc[::2], test.iloc[::4]], ignore_index=True)
    assert cand.duplicated().sum() >= len(test.iloc[::4])
    ks = [1, 5, 10]
    got = m.evaluate_candidates(sub, test, cand, ks=ks)
    # a candidate listed twice counts once: the reference ranks the distinct candidates
    ranked = m.predict_pairs(cand[cand.user_idx.isin(test.user_idx)].drop_duplicates(), sub, k=10)
    ref = MO.evaluate(ranked.user_idx, ranked.item_idx, ranked.relevance, test.user_idx, test.item_idx, ks)
    name = {"ndcg": "NDCG", "hitrate": "HitRate", "precision": "Precision", "recall": "Recall", "map": "MAP", "mrr": "MRR"}
    for mm, dct in ref.items():
        for k, v in dct.items():      # fp64 means summed in another order: the project's bound for metric means
            assert got[name[mm]][k] == pytest.approx(v, rel=1e-12, abs=1e-15), (mm, k)
    assert ref["hitrate"][10] > 0         # the held-out items do get ranked: the metrics see hits
    # the id block handed to the metrics, exactly: row i = the ranked frame of the i-th ground-truth user, -1 padded
    users, block = m.candidates_block(sub, test.user_idx.to_numpy(), cand, 10)
    block = block.cpu().numpy()
    assert users.tolist() == sorted(set(test.user_idx)) and block.shape == (len(users), 10) and block.dtype == np.int32
    exp = np.full_like(block, -1)
    for r, u in enumerate(users):
        it = ranked.item_idx[ranked.user_idx == u].to_numpy()
        exp[r, :len(it)] = it
    assert np.array_equal(block, exp)
    for u in (10_000, no_history):        # a cold user and a user without history: in the ground truth, empty rows
        assert u in set(test.user_idx) and np.all(block[users.tolist().index(u)] == -1)
    assert all(len(set(row[row >= 0])) == (row >= 0).sum() for row in block)          # unique items per row


# ---- 9. argument checks: on the host, before any HIP call (no GPU needed) ------------------------------------------------
def test_argument_checks_are_host_only():
    lib = N.load()
    fake = 0x1000            # never dereferenced: every call below is refused before the first HIP call
    nb = int(lib.cqlrec_pairs_topk_ws_bytes(4, 100, 128, 10))
    assert nb > 0
    assert lib.cqlrec_pairs_topk_ws_bytes(4, 100, 100, 10) == 0 and lib.cqlrec_pairs_topk_ws_bytes(4, 100, 128, 513) == 0
    assert N.PAIRS_MAX_K == 512
    assert lib.cqlrec_pairs_topk_ws_bytes((1 << 26) + 1, 100, 128, 10) == 0       # more rows than one launch can take

    def call(E=fake, d=128, k=10, ws_bytes=nb, outs=(fake, fake, fake), score=fake, seen=(None, None), n_sel=4):
        return lib.cqlrec_pairs_topk(fake, E, fake, 1000, d, fake, fake, None, n_sel, seen[0], seen[1], k, fake, ws_bytes, score,
                                     outs[0], outs[1], outs[2], None)
    for kwargs, msg in ((dict(d=100), "unsupported"), (dict(k=513), "out of range"), (dict(k=-1), "out of range"),
                        (dict(E=None), "NULL"), (dict(ws_bytes=nb - 1), "workspace too small"),
                        (dict(outs=(fake, None, fake)), "NULL"), (dict(k=0), "must be NULL"),
                        (dict(k=0, outs=(None, None, None), score=None), "out_score is NULL"),
                        (dict(seen=(fake, None)), "go together"), (dict(n_sel=(1 << 26) + 1), "n_sel=.*out of range")):
        with pytest.raises(N.CqlrecError, match=msg):
            N.check(call(**kwargs), "pairs_topk")
