"""The neighbourhood models on the GPU (replay_cql_amd.neighbour, csrc/neighbour.hip) against the yardstick
tests/neighbour_reference.py and the known answers of tests/golden/neighbour_known_answers.json.

Equality rules.  The engine is fed dyadic values (multiples of 2^-10, magnitude <= 2^6): every product and every sum is
exact in fp64 in any order, so ids, values and counts equal the yardstick's bit for bit, in both modes.  The plain model
(weighting None) on dyadic relevances is exact too: counts and sums are exact, and fp64 sqrt, multiply, add and divide
are correctly rounded on both sides.  The weighted models and the predictions are held to the bounds of
neighbour_reference.tolerance, and their top-k is checked as a certificate: every returned value is within tolerance of
the reference value of that pair, every admissible pair that is not returned has a reference value <= the k-th returned
value + tolerance, the count is min(k, admissible), and the returned rows are in their own order with the tie rule."""
import json
import math
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import neighbour_reference as NR
from replay_cql_amd import _native as N
from replay_cql_amd import neighbour as NB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "neighbour_known_answers.json").read_text())
DEFAULT = NB.DEFAULT_MAX_TUPLES
_CACHE = {}


# ------------------------------------------------------------------------------------------------- the engine
def dyadic(rng, n):
    """multiples of 2^-10 with magnitude <= 2^6, zero among them"""
    return rng.integers(-(1 << 16), (1 << 16) + 1, size=n).astype(np.float64) / 1024.0


def engine_case(n_cols):
    """L [n_q rows] and R [n_mid rows] with every shape the engine can meet; built once per n_cols"""
    if ("case", n_cols) in _CACHE:
        return _CACHE["case", n_cols]
    rng = np.random.default_rng(1000 + n_cols)
    n_q, n_mid, top = 50, 40, n_cols - 1
    R = []
    for m in range(n_mid):
        cols = rng.integers(0, n_cols, size=8)                       # duplicated columns inside a row occur
        R.append([(int(j), float(b)) for j, b in zip(cols, dyadic(rng, 8))])
    R[0] = [(j, float(b)) for j, b in zip(range(n_cols), dyadic(rng, n_cols))]   # reaches every column
    R[1] = [(top, 0.5)]                                               # the highest id, reached from every row
    R[5], R[n_mid - 1] = [], []                                       # empty R rows
    R[7] = [(11, 0.25), (top, -1.5)]
    R[8], R[9] = [(13, 2.0)], [(13, 2.0)]
    L = []
    for q in range(n_q):
        ms = [m for m in rng.integers(2, n_mid, size=6) if m not in (7, 8, 9)]
        L.append([(int(m), float(a)) for m, a in zip(ms, dyadic(rng, len(ms)))] + [(1, 1.0), (5, 3.0)])
    L[0] = [(0, 1.0)] + L[0]                                          # one row that reaches every column
    L[2] = [(7, float(a)) for a in dyadic(rng, 1500)] + [(1, 1.0)]    # (2, 11) and (2, top) have 1500 terms and more
    L[3], L[n_q - 1] = [], []                                         # empty L rows
    L[4] = [(8, 1.0), (9, -1.0), (1, 1.0)]                            # (4, 13) is reached and sums to 0
    norm_q = np.abs(dyadic(rng, n_q)) + 0.5
    norm_j = np.abs(dyadic(rng, n_cols)) + 0.5
    norm_q[10] = 0.0                                                  # a whole row of zero denominators when shrink = 0
    norm_j[[13, top, 20]] = 0.0
    mask = (rng.random(n_cols) < 0.7).astype(np.uint8)
    mask[top] = 1
    seen = [sorted(set(int(j) for j in rng.integers(0, n_cols, size=rng.integers(0, 12)))) for _ in range(n_q)]
    seen[6] = list(range(n_cols))                                     # removes every candidate of row 6
    seen[0] = list(range(0, n_cols, 2))
    case = dict(L=L, R=R, n_q=n_q, n_mid=n_mid, n_cols=n_cols, norm_q=norm_q, norm_j=norm_j, mask=mask, seen=seen)
    assert len(L[2]) * 2 > 4096 // 2 and max(len(r) for r in L) > 64
    _CACHE["case", n_cols] = case
    return case


def on_device(case):
    if "dev" not in case:
        t = lambda a: torch.as_tensor(a).to(DEV)
        case["dev"] = dict(L=tuple(t(a) for a in NR.csr(case["L"])), R=tuple(t(a) for a in NR.csr(case["R"])),
                           norm_q=t(case["norm_q"]), norm_j=t(case["norm_j"]), mask=t(case["mask"]),
                           seen=tuple(t(a) for a in NR.csr([[(j, 0.0) for j in s] for s in case["seen"]])[:2]))
    return case["dev"]


def run_engine(case, mode, k, max_tuples=DEFAULT, shrink=0.0, mask=False, seen=False):
    d = on_device(case)
    eng = NB.Neigh(torch.device(DEV))
    fit = mode == NR.FIT
    out = eng.topk(mode, d["L"], d["R"], case["n_mid"], case["n_cols"], k, max_tuples,
                   norm_q=d["norm_q"] if fit else None, norm_j=d["norm_j"] if fit else None, shrink=shrink,
                   mask=d["mask"] if mask else None, seen=d["seen"] if seen else None)
    return tuple(x.cpu().numpy() for x in out), eng.expansion


def ref_engine(case, mode, k, shrink=0.0, mask=False, seen=False):
    return NR.topk(case["L"], case["R"], k, mode, case["norm_q"], case["norm_j"], shrink,
                   case["mask"] if mask else None, case["seen"] if seen else None)


def same_bytes(got, ref, what):
    for g, r, name in zip(got, ref, ("ids", "vals", "count")):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape)
        assert g.tobytes() == r.tobytes(), (what, name, np.argwhere(g != r)[:5].tolist())


@pytest.mark.parametrize("k", [1, 10, 100, 1024])
@pytest.mark.parametrize("n_cols", [67, 1000])
def test_engine_fit_is_the_yardstick_bit_for_bit(n_cols, k):
    case = engine_case(n_cols)
    for shrink in (0.0, 0.5, 10.0):
        got, (total, largest) = run_engine(case, NR.FIT, k, shrink=shrink)
        ref = ref_engine(case, NR.FIT, k, shrink=shrink)
        same_bytes(got, ref, f"fit n_cols={n_cols} k={k} shrink={shrink}")
        ids, vals, count = got
        assert total == sum(len(case["R"][m]) for row in case["L"] for m, _ in row) and largest >= 3000
        assert count[3] == 0 and count[case["n_q"] - 1] == 0                       # empty L rows
        assert all(q not in ids[q] for q in range(case["n_q"]))                   # j == q is dropped
        for q in range(case["n_q"]):
            assert (ids[q, count[q]:] == -1).all() and (vals[q, count[q]:] == 0.0).all()
        if shrink == 0.0:
            assert count[10] == 0 and not np.isin(ids, [13, n_cols - 1, 20]).any()  # zero denominators are dropped
        else:
            assert count[10] > 0 and (k < 100 or 13 in ids[4])
        if k >= 100 and n_cols == 67:
            assert count.max() < k                                                 # k beyond the candidates
            assert count[0] == n_cols - (3 if shrink == 0.0 else 0) - 1            # row 0 reaches every column


@pytest.mark.parametrize("k", [1, 10, 100, 1024])
@pytest.mark.parametrize("n_cols", [67, 1000])
def test_engine_predict_is_the_yardstick_bit_for_bit(n_cols, k):
    case = engine_case(n_cols)
    for mask in (False, True):
        for seen in (False, True):
            got, _ = run_engine(case, NR.PREDICT, k, mask=mask, seen=seen)
            same_bytes(got, ref_engine(case, NR.PREDICT, k, mask=mask, seen=seen), f"predict {n_cols} {k} {mask} {seen}")
            ids, vals, count = got
            if seen:
                assert count[6] == 0                                               # its seen list holds every column
                assert not (set(ids[0, :count[0]]) & set(case["seen"][0]))
            elif not mask:
                assert count[0] == min(k, n_cols) and count[2] == min(k, 2)
                if k >= 2:                                                         # the reached zero sum is a candidate
                    assert 13 in ids[4] and vals[4][list(ids[4]).index(13)] == 0.0 and count[4] == 2
            if mask:
                assert case["mask"][ids[ids >= 0]].all()
            assert count[3] == 0 and (ids[3] == -1).all()


def test_engine_sums_1500_terms_exactly():
    case = engine_case(67)
    (ids, vals, count), _ = run_engine(case, NR.PREDICT, 67)
    terms = [a * 0.25 for m, a in case["L"][2] if m == 7]
    assert len(terms) == 1500 and vals[2][list(ids[2]).index(11)] == math.fsum(terms)


@pytest.mark.parametrize("mode", [NR.FIT, NR.PREDICT])
def test_engine_massive_ties_follow_the_modes_own_direction(mode):
    n_cols, n_mid, n_q, k = 67, 9, 30, 10
    R = [[(j, 1.0) for j in range(m, n_cols, 3)] for m in range(n_mid)]
    L = [[(q % n_mid, 1.0)] for q in range(n_q)]
    ones_q, ones_j = np.ones(n_q), np.ones(n_cols)
    t = lambda a: torch.as_tensor(a).to(DEV)
    eng = NB.Neigh(torch.device(DEV))
    fit = mode == NR.FIT
    got = eng.topk(mode, tuple(t(a) for a in NR.csr(L)), tuple(t(a) for a in NR.csr(R)), n_mid, n_cols, k, 64,
                   norm_q=t(ones_q) if fit else None, norm_j=t(ones_j) if fit else None, shrink=1.0)
    got = tuple(x.cpu().numpy() for x in got)
    same_bytes(got, NR.topk(L, R, k, mode, ones_q, ones_j, 1.0), f"ties mode={mode}")
    ids, vals, _ = got
    assert (vals == (0.5 if fit else 1.0)).all()
    step = np.diff(ids.astype(np.int64), axis=1)
    assert (step < 0).all() if fit else (step > 0).all()
    assert ids[0, 0] == (66 if fit else 0)                    # row 0 reaches 0, 3, ..., 66: the highest id is used


@pytest.mark.parametrize("mode", [NR.FIT, NR.PREDICT])
@pytest.mark.parametrize("n_cols", [67, 1000])
def test_engine_result_does_not_depend_on_max_tuples_nor_on_the_run(n_cols, mode):
    case = engine_case(n_cols)
    kw = dict(shrink=0.5) if mode == NR.FIT else dict(mask=True, seen=True)
    first, (total, largest) = run_engine(case, mode, 10, max_tuples=DEFAULT, **kw)
    assert largest > 64 and total > 4096                       # rows beyond the small budget; several chunks at 4 096
    for max_tuples in (64, 4096, DEFAULT):
        again, _ = run_engine(case, mode, 10, max_tuples=max_tuples, **kw)
        same_bytes(again, first, f"max_tuples={max_tuples} mode={mode} n_cols={n_cols}")


def test_engine_does_nothing_on_empty_input():
    eng = NB.Neigh(torch.device(DEV))
    z = lambda dt, n=0: torch.zeros(n, dtype=dt, device=DEV)
    ids, vals, count = eng.topk(NR.PREDICT, (z(torch.int64, 1), z(torch.int32), z(torch.float64)),
                                (z(torch.int64, 5), z(torch.int32), z(torch.float64)), 4, 7, 3, 64)
    assert ids.shape == (0, 3) and count.numel() == 0
    ids, vals, count = eng.topk(NR.PREDICT, (z(torch.int64, 4), z(torch.int32), z(torch.float64)),
                                (z(torch.int64, 5), z(torch.int32), z(torch.float64)), 4, 7, 3, 64)
    assert (ids.cpu() == -1).all() and (vals.cpu() == 0).all() and (count.cpu() == 0).all() and eng.expansion == (0, 0)


# ------------------------------------------------------------------------------------------------- the model
def model_log(kind="signed"):
    """about 300 users x 50 items with duplicated rows, an item nobody touched (20), and dyadic relevances; `signed`
    holds 0 and negative values and an item whose rows all weigh 0 (49)"""
    if ("log", kind) in _CACHE:
        return _CACHE["log", kind]
    rng = np.random.default_rng(7)
    user, item = [], []
    for u in range(300):
        if u in (17, 250):
            continue                                            # users without rows
        n = int(rng.integers(1, 13))
        its = rng.integers(0, 49, size=n)
        its = its[its != 20]
        user += [u] * len(its)
        item += [int(i) for i in its]
    user += [5, 5, 6]
    item += [49, 49, 49]
    user, item = np.array(user, dtype=np.int64), np.array(item, dtype=np.int64)
    order = rng.permutation(len(user))
    user, item = user[order], item[order]
    values = [0.0, -0.5, 0.25, 1.0, 2.0, 1.5, 3.0] if kind == "signed" else [0.5, 1.0, 2.0, 3.0, 0.25]
    rel = rng.choice(values, size=len(user))
    if kind == "signed":
        rel[item == 49] = 0.0
    log = {"user_idx": user, "item_idx": item, "relevance": rel, "timestamp": np.arange(len(user), dtype=np.int64)}
    _CACHE["log", kind] = log
    return log


def device_log(log):
    return {k: torch.as_tensor(v).to(DEV) for k, v in log.items()}


@pytest.mark.parametrize("use_relevance", [False, True])
def test_plain_model_is_the_yardstick_bit_for_bit(use_relevance):
    log = model_log("signed")
    n_users, n_items = int(log["user_idx"].max()) + 1, int(log["item_idx"].max()) + 1
    for shrink, max_tuples in ((0.0, DEFAULT), (2.5, 500)):
        model = NB.ItemKNN(10, use_relevance=use_relevance, shrink=shrink, max_tuples=max_tuples)
        model.fit(device_log(log))
        w = NR.weights(log["user_idx"], log["item_idx"], log["relevance"], use_relevance, None)
        assert model.row_weights.cpu().numpy().tobytes() == w.tobytes()
        assert model.item_norms.cpu().numpy().tolist() == NR.norms(log["item_idx"], w, n_items)
        ref = NR.similarity(log["user_idx"], log["item_idx"], w, n_users, n_items, 10, shrink)
        got = tuple(x.cpu().numpy() for x in model.similarity_device)
        same_bytes(got, ref, f"use_relevance={use_relevance} shrink={shrink}")
        assert got[2][20] == 0                                                  # an item nobody touched
        if use_relevance and shrink == 0.0:
            assert got[2][49] == 0 and not (got[0] == 49).any()                 # norm 0: every denominator is 0
            assert (w < 0).any() and (w == 0).any()                             # what went in
        frame = model.similarity
        assert list(frame.columns) == ["item_idx_one", "item_idx_two", "similarity"] and len(frame) == got[2].sum()
        assert frame["item_idx_one"].is_monotonic_increasing
        assert frame["item_idx_two"].tolist() == [int(j) for row, n in zip(got[0], got[2]) for j in row[:n]]
        assert model.fit_items["item_idx"].tolist() == sorted(set(log["item_idx"].tolist()))


def test_known_answers():
    case = GOLDEN["log"]
    frame = pd.DataFrame(case["rows"], columns=["user_idx", "item_idx", "relevance"]).astype({"user_idx": np.int64, "item_idx": np.int64})
    model = NB.ItemKNN(1, weighting=None)
    model.fit(frame)
    ids, vals, count = (x.cpu().numpy() for x in model.similarity_device)
    assert ids.tolist() == [[1], [0]] and count.tolist() == [1, 1]
    assert vals.tolist() == [[1.0 / (math.sqrt(2.0) * math.sqrt(2.0))]] * 2
    assert vals[0, 0] == pytest.approx(case["similarity_0_1"], rel=2.0 ** -51)
    recs = model.predict(frame, k=case["k"], users=case["users"])
    assert {str(u): int(i) for u, i in zip(recs["user_idx"], recs["item_idx"])} == case["recommended"]
    case = GOLDEN["weighting_log"]
    frame = pd.DataFrame(case["rows"], columns=["user_idx", "item_idx", "relevance"]).astype({"user_idx": np.int64, "item_idx": np.int64})
    for weighting in ("tf_idf", "bm25"):
        model = NB.ItemKNN(1, weighting=weighting)
        model.fit(frame)
        w = model.row_weights.cpu().numpy()
        for u, i, x in zip(frame["user_idx"], frame["item_idx"], w):
            tf = case["bm25"]["tf"][str(i)] if weighting == "bm25" else 1.0
            assert x == pytest.approx(tf * case[weighting]["idf"][str(u)], rel=1e-14)
        recs = model.predict(frame, k=case["k"], users=case["users"])
        assert recs.loc[recs["user_idx"] == 1, "item_idx"].iloc[0] == case[weighting]["recommended"]["1"]


def certificate(ids, vals, count, k, mode, ref, tol, what):
    """ref: per row {j: reference value} of the admissible pairs; tol(q, j): the absolute bound of that pair"""
    worst = 0.0
    for q, cand in enumerate(ref):
        n = int(count[q])
        assert n == min(k, len(cand)), (what, q, n, len(cand))
        got_ids, got_vals = [int(j) for j in ids[q, :n]], [float(v) for v in vals[q, :n]]
        assert (ids[q, n:] == -1).all() and (vals[q, n:] == 0.0).all(), (what, q)
        assert len(set(got_ids)) == n and all(j in cand for j in got_ids), (what, q, got_ids)
        for j, v in zip(got_ids, got_vals):
            t = tol(q, j)
            if t > 0.0:
                worst = max(worst, abs(v - cand[j]) / t)
            assert abs(v - cand[j]) <= t, (what, q, j, v, cand[j], t)
        for r in range(1, n):
            assert got_vals[r - 1] >= got_vals[r], (what, q, r)
            if got_vals[r - 1] == got_vals[r]:
                assert got_ids[r - 1] > got_ids[r] if mode == NR.FIT else got_ids[r - 1] < got_ids[r], (what, q, r)
        if n == k:
            for j, v in cand.items():
                if j not in got_ids:
                    assert v <= got_vals[-1] + tol(q, j), (what, q, j, v, got_vals[-1])
    return worst


@pytest.mark.parametrize("use_relevance", [False, True])
@pytest.mark.parametrize("weighting", ["tf_idf", "bm25"])
def test_weighted_model(weighting, use_relevance):
    log = model_log("positive")
    n_users, n_items = int(log["user_idx"].max()) + 1, int(log["item_idx"].max()) + 1
    model = NB.ItemKNN(10, use_relevance=use_relevance, shrink=0.5, weighting=weighting, max_tuples=700)
    model.fit(device_log(log))
    w = model.row_weights.cpu().numpy()
    ref_w = NR.weights(log["user_idx"], log["item_idx"], log["relevance"], use_relevance, weighting)
    ratio = np.abs(w - ref_w) / np.array([NR.tolerance("weight", x) for x in ref_w])
    print(f"weights {weighting} use_relevance={use_relevance}: worst |got - ref| / bound = {ratio.max():.3f}")
    assert (w >= 0).all() and ratio.max() <= 1.0
    by_item, by_user = NR.log_views(log["user_idx"], log["item_idx"], w, n_users, n_items)
    nrm = NR.norms(log["item_idx"], w, n_items)
    terms = NR.product(by_item, by_user)
    ref = [NR.candidates(t, NR.FIT, q, nrm, nrm, 0.5) for q, t in enumerate(terms)]
    rows = np.bincount(log["item_idx"], minlength=n_items)
    tol = lambda q, j: NR.tolerance("similarity", ref[q][j], terms=len(terms[q][j]), n_i=int(rows[q]), n_j=int(rows[j]))
    ids, vals, count = (x.cpu().numpy() for x in model.similarity_device)
    worst = certificate(ids, vals, count, 10, NR.FIT, ref, tol, f"{weighting} {use_relevance}")
    print(f"similarity {weighting} use_relevance={use_relevance}: worst |got - ref| / bound = {worst:.3f}")
    assert np.abs(model.item_norms.cpu().numpy() - np.array(nrm)).max() <= 64 * 2.0 ** -53 * max(nrm)


def fitted_model():
    if "model" not in _CACHE:
        model = NB.ItemKNN(8, use_relevance=True, shrink=1.0, weighting="bm25", max_tuples=900)
        model.fit(device_log(model_log("positive")))
        _CACHE["model"] = (model, NR.table(*(x.cpu().numpy() for x in model.similarity_device)))
    return _CACHE["model"]


def predict_log():
    """another log than the fit log: other rows, new users (300 .. 309), items without a similarity row (50 .. 54)"""
    if "plog" not in _CACHE:
        rng = np.random.default_rng(11)
        user = rng.integers(0, 310, size=1500)
        user = user[(user != 33)]                                           # 33 has no rows here
        item = rng.integers(0, 55, size=len(user))
        _CACHE["plog"] = {"user_idx": user.astype(np.int64), "item_idx": item.astype(np.int64)}
    return _CACHE["plog"]


def predict_reference(sim, log, users, items, filter_seen):
    """(per user {j: reference score} of the admissible pairs, the absolute bound of every pair)"""
    terms = NR.predict_terms(sim, log["user_idx"], log["item_idx"], users)
    seen = {}
    for u, i in zip(log["user_idx"], log["item_idx"]):
        seen.setdefault(int(u), set()).add(int(i))
    items = set(int(j) for j in items)
    ref, tol = [], []
    for u in users:
        adm = {j: ts for j, ts in terms[int(u)].items() if j in items and not (filter_seen and j in seen.get(int(u), ()))}
        ref.append({j: math.fsum(ts) for j, ts in adm.items()})
        tol.append({j: NR.tolerance("score", terms=len(ts), sum_abs=math.fsum(abs(t) for t in ts)) for j, ts in adm.items()})
    return ref, tol


def block_of(out, users, k):
    """the device columns of `recommend` as (ids, vals, count) blocks in the order of `users`"""
    u, i, v = (out[c].cpu().numpy() for c in ("user_idx", "item_idx", "relevance"))
    assert (u.dtype, i.dtype, v.dtype) == (np.int32, np.int32, np.float64)
    ids, vals = np.full((len(users), k), -1, dtype=np.int32), np.zeros((len(users), k))
    count = np.zeros(len(users), dtype=np.int32)
    pos = {int(x): r for r, x in enumerate(users)}
    last = -1
    for uu, ii, vv in zip(u, i, v):
        r = pos[int(uu)]
        assert r >= last                                                   # users in the order given, then rank
        last = r
        ids[r, count[r]], vals[r, count[r]] = ii, vv
        count[r] += 1
    return ids, vals, count


@pytest.mark.parametrize("filter_seen", [True, False])
@pytest.mark.parametrize("which", ["fit_log", "other_log"])
@pytest.mark.parametrize("k", [5, 60])
def test_recommend_certificate(k, which, filter_seen):
    model, sim = fitted_model()
    log = model_log("positive") if which == "fit_log" else predict_log()
    users = sorted(set(int(u) for u in log["user_idx"]))
    items = list(range(50))
    out = model.recommend(device_log(log), k, filter_seen_items=filter_seen)
    ref, tol = predict_reference(sim, log, users, items, filter_seen)
    ids, vals, count = block_of(out, users, k)
    worst = certificate(ids, vals, count, k, NR.PREDICT, ref, lambda q, j: tol[q][j], f"recommend {which} k={k}")
    print(f"recommend {which} k={k} filter_seen={filter_seen}: worst |got - ref| / bound = {worst:.3f}")
    assert model.expansion[0] > 900                                         # several chunks at this model's max_tuples
    if k == 60:
        assert count.max() < k                                              # k larger than what a user can get
    # subsets: some users (a cold one and one without rows among them, in an order of their own) and half the items
    users = [299, 3, 999, 33, 305, 8, 250] + list(range(40, 60))
    items = list(range(0, 50, 2)) + [52, 77]
    out = model.recommend(device_log(log), k, users=torch.tensor(users), items=items, filter_seen_items=filter_seen)
    ref, tol = predict_reference(sim, log, users, items, filter_seen)
    ids, vals, count = block_of(out, users, k)
    certificate(ids, vals, count, k, NR.PREDICT, ref, lambda q, j: tol[q][j], f"recommend subset {which} k={k}")
    assert count[users.index(999)] == 0 and (ids[ids >= 0] % 2 == 0).all()


@pytest.mark.parametrize("filter_seen", [True, False])
def test_predict_on_pandas_equals_recommend(filter_seen):
    model, sim = fitted_model()
    log = predict_log()
    frame = pd.DataFrame(log)
    users, items, k = sorted([299, 3, 999, 33, 305, 8] + list(range(40, 60))), list(range(0, 50, 2)), 7
    recs = model.predict(frame, k, users=users, items=items, filter_seen_items=filter_seen)
    assert isinstance(recs, pd.DataFrame) and list(recs.columns) == ["user_idx", "item_idx", "relevance"]
    assert [str(t) for t in recs.dtypes] == ["int32", "int32", "float64"]
    out = model.recommend(device_log(log), k, users=users, items=items, filter_seen_items=filter_seen)
    for c in recs.columns:
        assert recs[c].to_numpy().tobytes() == out[c].cpu().numpy().tobytes(), c
    assert recs.groupby("user_idx").size().max() <= k and 999 not in set(recs["user_idx"])
    ref, tol = predict_reference(sim, log, users, items, filter_seen)
    ids, vals, count = block_of(out, users, k)
    certificate(ids, vals, count, k, NR.PREDICT, ref, lambda q, j: tol[q][j], "predict pandas")
    # every user of the log, every fitted item
    recs = model.predict(frame, 3, filter_seen_items=filter_seen)
    out = model.recommend(frame, 3, items=model.fit_items["item_idx"], filter_seen_items=filter_seen)
    assert recs["item_idx"].to_numpy().tobytes() == out["item_idx"].cpu().numpy().tobytes()
    assert recs["relevance"].to_numpy().tobytes() == out["relevance"].cpu().numpy().tobytes()


def test_predict_pairs():
    model, sim = fitted_model()
    log = predict_log()
    rng = np.random.default_rng(3)
    pairs = pd.DataFrame({"user_idx": rng.integers(0, 312, size=400), "item_idx": rng.integers(0, 50, size=400)}).drop_duplicates()
    pairs = pd.concat([pairs, pd.DataFrame({"user_idx": [999, 33], "item_idx": [1, 2]})], ignore_index=True)
    got = model.predict_pairs(pairs, pd.DataFrame(log))
    assert [str(t) for t in got.dtypes] == ["int32", "int32", "float64"]
    known = pairs[pairs["item_idx"].isin(model.fit_items["item_idx"])]     # the template drops cold items
    ref = NR.pair_scores(sim, log["user_idx"], log["item_idx"], list(zip(known["user_idx"], known["item_idx"])))
    terms = NR.predict_terms(sim, log["user_idx"], log["item_idx"], set(int(u) for u in known["user_idx"]))
    want = {(int(u), int(j)): r for (u, j), r in zip(zip(known["user_idx"], known["item_idx"]), ref) if r is not None}
    assert 0 < len(want) < len(known) and (999, 1) not in want
    assert [(int(u), int(j)) for u, j in zip(got["user_idx"], got["item_idx"])] == list(want)
    for u, j, v in zip(got["user_idx"], got["item_idx"], got["relevance"]):
        ts = terms[int(u)][int(j)]
        assert abs(v - want[int(u), int(j)]) <= NR.tolerance("score", terms=len(ts), sum_abs=math.fsum(abs(t) for t in ts))
    top = model.predict_pairs(pairs, pd.DataFrame(log), k=2)
    assert top.groupby("user_idx").size().max() == 2 and len(top) < len(got)
    with pytest.raises(ValueError, match="log is not provided"):
        model.predict_pairs(pairs)


def test_get_nearest_items():
    model, sim = fitted_model()
    items, k = [0, 3, 7, 20, 48], 3

    def expected(candidates):
        rows = []
        for i in items:
            near = [(j, s) for j, s in sim[i] if candidates is None or j in candidates]
            rows += [(i, j, s) for j, s in sorted(near, key=lambda t: (-t[1], -t[0]))[:k]]
        return rows

    for metric in (None, "anything"):
        got = model.get_nearest_items(items, k, metric=metric)
        assert list(got.columns) == ["item_idx", "neighbour_item_idx", "similarity"]
        assert [str(t) for t in got.dtypes] == ["int32", "int32", "float64"]
        assert list(got.itertuples(index=False, name=None)) == expected(None)
    cand = list(range(0, 50, 3))
    got = model.get_nearest_items(pd.DataFrame({"item_idx": items}), k, candidates=cand)
    assert list(got.itertuples(index=False, name=None)) == expected(set(cand)) and 0 < len(got) < 15
    assert 20 not in set(got["item_idx"])


def test_the_frame_predict_returns_scores_as_a_baseline():
    from replay_cql_amd.metrics import NDCG
    model, _ = fitted_model()
    frame = pd.DataFrame(model_log("positive"))
    recs = model.predict(frame, 5, filter_seen_items=False)
    truth = frame[["user_idx", "item_idx", "relevance"]].drop_duplicates(["user_idx", "item_idx"])
    value = NDCG()(recs, truth, 5)
    assert 0.0 < float(value) <= 1.0


def test_fit_rejects_nan_relevance_and_large_k():
    log = {k: v.copy() for k, v in model_log("positive").items()}
    log["relevance"][3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        NB.ItemKNN(use_relevance=True).fit(device_log(log))
    NB.ItemKNN(use_relevance=False).fit(device_log(log))                   # the column is not read
    with pytest.raises(ValueError, match="num_neighbours"):
        NB.ItemKNN(N.NEIGHBOUR_MAX_K + 1).fit(device_log(log))
