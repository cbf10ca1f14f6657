"""Association rules on the GPU (replay_cql_amd.association_rules, section f10 of csrc/neighbour.hip) against the
yardstick tests/rules_reference.py and the known answers of tests/golden/association_rules_known_answers.json.

Equality rules.  On count data every sum is an integer and each measure is a chain of single IEEE operations in the
normative order, so ids, the three planes and the counts equal the yardstick's bit for bit.  The same holds for dyadic
relevances (multiples of 2^-3, magnitude <= 2^4: every sum is exact in any order).  On other non-negative relevances
confidence and lift are held to rules_reference.tolerance; the confidence gain is not compared there (its differences
cancel).  Predictions are neighbour_reference's on the chosen plane, fed the device's table."""
import json
import math
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import neighbour_reference as NR
import rules_reference as RR
from replay_cql_amd import _native as N
from replay_cql_amd import neighbour as NB
from replay_cql_amd.association_rules import AssociationRulesItemRec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "association_rules_known_answers.json").read_text())
KNN_GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "neighbour_known_answers.json").read_text())
PLANES = ("ids", "confidence", "lift", "confidence_gain", "count")
_CACHE = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def frame(session, item, relevance, session_col="user_idx", **more):
    return pd.DataFrame({session_col: session, "item_idx": item, "relevance": relevance, **more})


def as_arrow(df):
    import pyarrow as pa
    return pa.Table.from_pandas(df, preserve_index=False)


def as_device(df):
    return {c: torch.as_tensor(df[c].to_numpy()).to(DEV) for c in df.columns}


def fitted(df, **args):
    model = AssociationRulesItemRec(**args)
    model.fit(df)
    return model


def device_table(model):
    return tuple(x.cpu().numpy() for x in model.similarity_device)


def same_bytes(got, ref, what):
    for g, r, name in zip(got, ref, PLANES):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.dtype, r.shape)
        assert g.tobytes() == r.tobytes(), (what, name, np.argwhere(g != r)[:5].tolist())


def padded(table):
    ids, conf, lift, gain, count = table
    for a in range(len(count)):
        assert (ids[a, count[a]:] == -1).all() and (ids[a, :count[a]] >= 0).all()
        for plane in (conf, lift, gain):
            assert (plane[a, count[a]:] == 0.0).all()


# ------------------------------------------------------------------------------------------------- known answers
def test_golden_docstring_log_through_every_kind_of_log():
    case = GOLDEN["docstring"]
    df = pd.DataFrame(case["log"]).astype({"user_idx": np.int64, "item_idx": np.int64})
    tables = []
    for log in (df, as_arrow(df), as_device(df)):
        model = fitted(log, **case["args"])
        tables.append(device_table(model))
        sim = model.similarity
        assert list(sim.columns) == ["item_idx_one", "item_idx_two", "confidence", "lift", "confidence_gain"]
        assert sim.to_dict("records") == case["similarity"]
        assert model.get_similarity is sim and model._dataframes["similarity"] is sim
        pairs = pd.DataFrame(case["predict_pairs"]["pairs"])
        for metric in ("confidence", "lift"):
            model.similarity_metric = metric
            out = model.predict_pairs(pairs, df)
            assert out["relevance"].tolist() == case["predict_pairs"][metric]
            assert out["user_idx"].tolist() == [2] and out["item_idx"].tolist() == [1]
    same_bytes(tables[1], tables[0], "arrow")
    same_bytes(tables[2], tables[0], "device")


def test_golden_fixture_log_plain_and_with_relevance():
    case = GOLDEN["fixture"]
    df = pd.DataFrame(case["log"]).astype({"user_idx": np.int64, "item_idx": np.int64})
    for key, use in (("plain", False), ("use_relevance", True)):
        want = case[key]
        tables = []
        for log in (df, as_arrow(df), as_device(df)):
            model = fitted(log, use_relevance=use, **case["args"])
            tables.append(device_table(model))
            assert model.num_sessions == case["num_sessions"]
            assert int(model.item_count.sum().item()) == want["distinct_rows"]      # user 3's item 0: two rows or one
            a, b = want["pair"]
            row = model.similarity.query(f"item_idx_one == {a} and item_idx_two == {b}")
            assert len(row) == 1
            for metric in RR.METRICS:
                assert row[metric].iloc[0] == want["expected"][metric], (key, metric)
            rel = model.item_relevance.cpu().numpy()
            assert [rel[a], rel[b]] == want["counts"][:2]
        same_bytes(tables[1], tables[0], key + " arrow")
        same_bytes(tables[2], tables[0], key + " device")
        ref = RR.table(df["user_idx"], df["item_idx"], df["relevance"], 4, 1000, 1, 1, use)
        same_bytes(tables[0], ref, key)
    model = fitted(df, **case["args"])
    for q in case["nearest"]:
        out = model.get_nearest_items(q["items"], q["k"], q["metric"], candidates=q["candidates"])
        assert list(out.columns) == ["item_idx", "neighbour_item_idx", q["metric"]] and len(out) == q["rows"]
        if "values" in q:
            assert out[q["metric"]].tolist() == q["values"]
    with pytest.raises(ValueError, match=r"^Select one of the valid distance metrics: \['lift', 'confidence', 'confidence_gain'\]$"):
        model.get_nearest_items([2], 1, "invalid")
    with pytest.raises(ValueError, match=r"^Select one of the valid metrics for predict: "):
        model.similarity_metric = "invalid"


# ------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("min_item_count", [1, 4])
@pytest.mark.parametrize("min_pair_count", [0, 1, 3])
@pytest.mark.parametrize("k", [1, 3, 10])
def test_count_data_is_the_yardstick_bit_for_bit(k, min_pair_count, min_item_count):
    session, item, rel, n_items = cached("count", RR.count_log)
    log = cached("count_dev", lambda: as_device(frame(session, item, rel)))
    model = fitted(log, num_neighbours=k, min_pair_count=min_pair_count, min_item_count=min_item_count)
    got = device_table(model)
    ref = RR.table(session, item, rel, n_items, k, min_item_count, min_pair_count)
    same_bytes(got, ref, f"count k={k} pairs>={min_pair_count} items>={min_item_count}")
    padded(got)
    ids, count = got[0], got[4]
    assert ids[57, 0] == 59 and ids[58, 0] == 59 and ids[59, 0] == 58          # the tie at the cut: the larger id
    assert all(a not in ids[a] for a in range(n_items))
    assert (count[50] == 0) == (min_item_count == 4) and count[51] > 0 and count[52] > 0
    kept = set(ids[53, :count[53]].tolist()) & {54, 55, 56}
    if k == 10 and min_item_count == 1:
        assert kept == {0: {54, 55, 56}, 1: {54, 55, 56}, 3: {55, 56}}[min_pair_count]
    total, largest = model.expansion
    assert total > 0 and largest > 0


@pytest.mark.parametrize("max_tuples", [1, 64, None])
def test_dyadic_relevances_are_bit_for_bit_whatever_max_tuples(max_tuples):
    session, item, rel, n_items = cached("dyadic", RR.dyadic_log)
    log = cached("dyadic_dev", lambda: as_device(frame(session, item, rel)))
    more = {} if max_tuples is None else {"max_tuples": max_tuples}
    model = fitted(log, num_neighbours=10, min_item_count=1, min_pair_count=1, use_relevance=True, **more)
    got = device_table(model)
    ref = cached("dyadic_ref", lambda: RR.table(session, item, rel, n_items, 10, 1, 1, True))
    same_bytes(got, ref, f"dyadic max_tuples={max_tuples}")
    padded(got)
    ids, conf, lift, gain, count = got
    assert model.expansion[1] > 64                                             # a row larger than max_tuples
    assert count[40] == 0 and not (ids == 40).any()                            # relevance sums to 0: no pair either way
    assert model.item_relevance[40].item() == 0.0
    r = ids[41].tolist().index(42)
    assert gain[41, r] == math.inf and math.isfinite(lift[41, r])              # C - p == 0
    counts, pair_terms = RR.term_counts(session, item, rel)
    assert [pair_terms[a, a + 1] for a in (41, 43, 45, 47)] == [32, 33, 64, 65]
    for a in (41, 43, 45, 47):
        assert a + 1 in ids[a] and a in ids[a + 1]
    rows = RR.distinct_rows(session, item, rel, True)
    assert [r for r in rows if r[:2] == (0, 1)] == [(0, 1, 1.5), (0, 1, 3.0)]     # two relevances, the duplicate gone
    assert int(model.item_count[1].item()) == counts[1]


def test_num_neighbours_none_keeps_every_pair_and_the_limit_is_named():
    session, item, rel, n_items = cached("count", RR.count_log)
    log = cached("count_dev", lambda: as_device(frame(session, item, rel)))
    model = fitted(log, num_neighbours=None, min_item_count=1, min_pair_count=1)
    got = device_table(model)
    assert got[0].shape == (n_items, n_items - 1)
    same_bytes(got, RR.table(session, item, rel, n_items, None, 1, 1), "num_neighbours=None")
    with pytest.raises(ValueError, match="1024"):
        fitted(log, num_neighbours=1025)
    with pytest.raises(ValueError, match="1024"):
        fitted(log, num_neighbours=0)
    wide = {"user_idx": torch.tensor([0, 0], device=DEV), "item_idx": torch.tensor([0, 1026], device=DEV)}
    with pytest.raises(ValueError, match="limit of 1024"):
        fitted(wide, num_neighbours=None, min_item_count=1)
    bad = as_device(frame(session[:4], item[:4], np.array([1.0, np.nan, 1.0, 1.0])))
    with pytest.raises(ValueError, match="NaN or an infinite"):
        fitted(bad, use_relevance=True)
    bad = as_device(frame(session[:4], item[:4], np.array([1.0, np.inf, 1.0, 1.0])))
    with pytest.raises(ValueError, match="NaN or an infinite"):
        fitted(bad, use_relevance=True)
    fitted(bad, use_relevance=False, min_item_count=1)                          # the column is not read then


def test_session_col_groups_the_fit_and_predict_still_sums_by_user():
    session, item, rel, n_items = cached("dyadic", RR.dyadic_log)
    user = (session * 7 + item) % 31                                            # unrelated to the sessions
    df = frame(session, item, rel, session_col="session", user_idx=user)
    model = fitted(as_device(df), session_col="session", num_neighbours=10, min_item_count=1, min_pair_count=1,
                   use_relevance=True, similarity_metric="lift")
    got = device_table(model)
    same_bytes(got, cached("dyadic_ref", lambda: RR.table(session, item, rel, n_items, 10, 1, 1, True)), "session_col")
    by_user = fitted(as_device(df), num_neighbours=10, min_item_count=1, min_pair_count=1, use_relevance=True)
    assert device_table(by_user)[0].tobytes() != got[0].tobytes()
    sim = NR.table(got[0], got[2], got[4])
    check_recs(model.predict(df, 5), sim, user, item, sorted(set(user.tolist())), range(n_items), 5, True)


# ------------------------------------------------------------------------------------------------- tolerance
def test_non_dyadic_relevances_within_the_bound_of_the_sums():
    rng = np.random.default_rng(21)
    session, item, _, n_items = cached("count", RR.count_log)
    rel = rng.random(len(session)) * 5.0 + 0.01
    model = fitted(as_device(frame(session, item, rel)), num_neighbours=n_items, min_item_count=1, min_pair_count=1,
                   use_relevance=True)
    ids, conf, lift, gain, count = device_table(model)
    r_ids, r_conf, r_lift, _, r_count = RR.table(session, item, rel, n_items, n_items, 1, 1, True)
    counts, pair_terms = RR.term_counts(session, item, rel)
    assert count.tolist() == r_count.tolist() and count.max() < n_items         # nothing is cut
    worst = 0.0
    for a in range(n_items):
        ref = {int(b): (r_conf[a, r], r_lift[a, r]) for r, b in enumerate(r_ids[a, :r_count[a]])}
        assert set(ids[a, :count[a]].tolist()) == set(ref)
        for r in range(count[a]):
            b = int(ids[a, r])
            tol = RR.tolerance(counts[a], counts[b], pair_terms[a, b])
            for got, want in ((conf[a, r], ref[b][0]), (lift[a, r], ref[b][1])):
                worst = max(worst, abs(got - want) / (tol * abs(want)))
        assert (np.diff(lift[a, :count[a]]) <= 0).all()
    print(f"confidence / lift: worst error over bound = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- predict
def check_recs(recs, sim, log_user, log_item, users, items, k, filter_seen):
    """A frame of recommendations as a certificate against neighbour_reference.predict_terms: every user has min(k,
    admissible) rows; each score is within the bound of its sum of the reference (equal where infinite); the rows are in
    their own order, ties by item ascending; no admissible item left out beats the last row by more than its bound."""
    got = {}
    for u, j, s in zip(recs["user_idx"], recs["item_idx"], recs["relevance"]):
        got.setdefault(int(u), []).append((int(j), float(s)))
    assert set(got) <= set(int(u) for u in users)
    terms = NR.predict_terms(sim, log_user, log_item, users)
    seen = {}
    for u, i in zip(log_user, log_item):
        seen.setdefault(int(u), set()).add(int(i))
    items = set(int(j) for j in items)
    for u in users:
        adm = {j: ts for j, ts in terms[int(u)].items() if j in items and not (filter_seen and j in seen.get(int(u), ()))}
        ref = {j: math.fsum(ts) for j, ts in adm.items()}
        tol = {j: NR.tolerance("score", terms=len(ts), sum_abs=math.fsum(abs(t) for t in ts)) for j, ts in adm.items()}
        rows = got.get(int(u), [])
        ids, vals = [j for j, _ in rows], [s for _, s in rows]
        assert len(rows) == min(k, len(adm)), (u, len(rows), len(adm))
        assert len(set(ids)) == len(ids) and all(j in adm for j in ids), (u, ids)
        for j, s in rows:
            assert s == ref[j] if math.isinf(ref[j]) else abs(s - ref[j]) <= tol[j], (u, j, s, ref[j])
        for r in range(1, len(rows)):
            assert vals[r - 1] >= vals[r] and (vals[r - 1] != vals[r] or ids[r - 1] < ids[r]), (u, r)
        if len(rows) == k:
            assert all(v <= vals[-1] + tol[j] for j, v in ref.items() if j not in ids), u


def test_predict_recommend_and_pairs_follow_the_metric():
    session, item, rel, n_items = cached("dyadic", RR.dyadic_log)
    df = frame(session, item, rel)
    log = cached("dyadic_dev", lambda: as_device(df))
    model = fitted(log, num_neighbours=10, min_item_count=1, min_pair_count=1, use_relevance=True)
    table = device_table(model)
    before = [x.tobytes() for x in table]
    users = list(range(0, 270, 3)) + [100000]
    subset = [j for j in range(n_items) if j % 3]
    seen_frames = {}
    for plane, metric in ((1, "confidence"), (2, "lift"), (3, "confidence_gain")):
        model.similarity_metric = metric
        sim = NR.table(table[0], table[plane], table[4])
        for filter_seen in (True, False):
            for items in (None, subset):
                recs = model.predict(df, 7, users=users, items=items, filter_seen_items=filter_seen)
                check_recs(recs, sim, session, item, users, range(n_items) if items is None else items, 7, filter_seen)
                seen_frames[metric, filter_seen, items is None] = recs
        out = model.recommend(log, 7, users=users)
        assert (out["user_idx"].dtype, out["item_idx"].dtype, out["relevance"].dtype) == (torch.int32, torch.int32, torch.float64)
        check_recs({c: out[c].cpu().numpy() for c in out}, sim, session, item, users, range(n_items), 7, True)
        assert (np.diff([users.index(int(u)) for u in out["user_idx"].cpu()]) >= 0).all()      # in the order of `users`
        pairs = [(u, j) for u in users[:40] for j in (0, 1, 42, 44, 40)]
        want = NR.pair_scores(sim, session, item, pairs)
        terms = NR.predict_terms(sim, session, item, users[:40])
        got = model.predict_pairs(pd.DataFrame(pairs, columns=["user_idx", "item_idx"]), df)
        kept = [(p, w) for p, w in zip(pairs, want) if w is not None]
        assert list(zip(got["user_idx"], got["item_idx"])) == [p for p, _ in kept] and len(kept) > 10
        for s, ((u, j), w) in zip(got["relevance"], kept):
            ts = terms[u][j]
            bound = NR.tolerance("score", terms=len(ts), sum_abs=math.fsum(abs(t) for t in ts))
            assert s == w if math.isinf(w) else abs(s - w) <= bound, (u, j)
    # the metric changes the result, not the table
    a, b = seen_frames["confidence", True, True], seen_frames["lift", True, True]
    assert a["relevance"].tolist() != b["relevance"].tolist()
    assert [x.tobytes() for x in device_table(model)] == before
    # +inf gains flow through the sums and rank first
    gain = seen_frames["confidence_gain", False, True]
    infinite = gain[np.isinf(gain["relevance"])]
    assert len(infinite) and (infinite["relevance"] > 0).all()
    for u, rows in gain.groupby("user_idx"):
        flags = np.isinf(rows["relevance"].to_numpy())
        assert not flags.any() or flags[:flags.sum()].all()


# ------------------------------------------------------------------------------------------------- the edges
def test_a_long_run_of_one_session_item_is_made_distinct_in_linear_time():
    session, item, rel, n_items = cached("dyadic", RR.dyadic_log)
    n = 1 << 18
    long_rel = np.where(np.arange(n) % 3 == 0, 2.5, 0.75)
    s = np.concatenate([np.zeros(n, dtype=np.int64), session])
    i = np.concatenate([np.full(n, 2, dtype=np.int64), item])
    w = np.concatenate([long_rel, rel])
    order = np.random.default_rng(5).permutation(len(s))
    s, i, w = s[order], i[order], w[order]
    model = fitted(as_device(frame(s, i, w)), num_neighbours=10, min_item_count=1, min_pair_count=1, use_relevance=True)
    same_bytes(device_table(model), RR.table(s, i, w, n_items, 10, 1, 1, True), "long run")
    assert int(model.item_count.sum().item()) == len(RR.distinct_rows(s, i, w, True)) < len(session) + 3


def test_empty_outcomes_are_tables_not_errors():
    session, item, rel, n_items = cached("count", RR.count_log)
    log = cached("count_dev", lambda: as_device(frame(session, item, rel)))
    model = fitted(log, min_item_count=10 ** 6, num_neighbours=5)
    ids, conf, lift, gain, count = device_table(model)
    assert ids.shape == (n_items, 5) and (ids == -1).all() and (count == 0).all()
    assert not conf.any() and not lift.any() and not gain.any()
    assert len(model.similarity) == 0 and model.expansion == (0, 0)
    assert len(model.predict(frame(session, item, rel), 3)) == 0
    assert model.recommend(log, 3)["item_idx"].numel() == 0
    assert len(model.get_nearest_items([1, 2], 3)) == 0
    # an item alone in its sessions has no partner
    lonely = as_device(frame(np.array([0, 0, 1, 2, 2]), np.array([0, 1, 2, 0, 1]), np.ones(5)))
    model = fitted(lonely, min_item_count=1, min_pair_count=1, num_neighbours=3)
    ids, _, _, _, count = device_table(model)
    assert count.tolist() == [1, 1, 0] and (ids[2] == -1).all() and ids[0, 0] == 1 and ids[1, 0] == 0


def test_item_knn_is_unchanged_by_the_shared_chunk_loop():
    case = KNN_GOLDEN["log"]
    knn_frame = pd.DataFrame(case["rows"], columns=["user_idx", "item_idx", "relevance"]).astype(
        {"user_idx": np.int64, "item_idx": np.int64})
    session, item, rel, n_items = cached("dyadic", RR.dyadic_log)
    log = cached("dyadic_dev", lambda: as_device(frame(session, item, rel)))

    def knn():
        small = NB.ItemKNN(1, weighting=None)
        small.fit(knn_frame)
        big = NB.ItemKNN(10, use_relevance=True, shrink=0.5, max_tuples=64)
        big.fit(log)
        return [x.cpu().numpy() for x in small.similarity_device], [x.cpu().numpy() for x in big.similarity_device]
    small_0, big_0 = knn()
    fitted(log, num_neighbours=10, min_item_count=1, min_pair_count=1, use_relevance=True)
    small_1, big_1 = knn()
    for a, b in zip(small_0 + big_0, small_1 + big_1):
        assert a.tobytes() == b.tobytes()
    assert small_1[0].tolist() == [[1], [0]] and small_1[2].tolist() == [1, 1]
    assert small_1[1].tolist() == [[1.0 / (math.sqrt(2.0) * math.sqrt(2.0))]] * 2
    # dyadic weights: the plain model is exact, so the yardstick gives the same bytes
    ref = NR.similarity(session, item, rel, int(session.max()) + 1, n_items, 10, 0.5)
    for g, r in zip(big_1, ref):
        assert g.tobytes() == r.tobytes()
