"""The extended metrics on the GPU (replay_cql_amd.metrics, csrc/metrics.hip): the reference's known answers through the
public classes, the relations its tests state, random frames and one large block against tests/metrics_reference.py,
and CQL.evaluate(extra=...) against the classes.

Bounds: known answers rel=1e-12, abs=1e-15 (the project's bound for them, tests/test_metrics_oracle.py); per-user values
rtol=1e-13, atol=1e-15 and means rel=1e-12 (tests/test_gpu_prep.py, the same fp64 arithmetic); integers are equal.  The
confidence interval holds a standard deviation rounded to float32, so two correct evaluations of it may land on
neighbouring float32 values: rel=2**-22."""
import json
import math
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import cql_oracle as O
from replay_cql_amd import metrics as M
from tests import metrics_reference as R

pytestmark = pytest.mark.gpu

KA = json.loads((Path(__file__).resolve().parent / "golden" / "metrics_known_answers.json").read_text())
FX = KA["fixtures"]
TOL = dict(rel=1e-12, abs=1e-15)
QUALITY = {n: getattr(M, n) for n in KA["quality_metrics"]}
DEV = "cuda:0"


def df(rows):
    a = np.asarray(rows, np.float64).reshape(-1, 3)
    return pd.DataFrame({"user_idx": a[:, 0].astype(np.int32), "item_idx": a[:, 1].astype(np.int32), "relevance": a[:, 2]})


def users_df(ids):
    return pd.DataFrame({"user_idx": np.asarray(ids, np.int32)})


def _gt_users(spec):
    if spec is None:
        return None
    return users_df(FX[spec] if isinstance(spec, str) else spec)


def _make(call):
    m = call["metric"]
    if m in ("Surprisal", "Unexpectedness", "Coverage"):
        return getattr(M, m)(df(FX[call["init"]]))
    return getattr(M, m)()


@pytest.mark.parametrize("call", KA["calls"], ids=[c["id"] for c in KA["calls"]])
def test_known_answers_of_whole_calls(call):
    metric, k, gu = _make(call), call["k"], _gt_users(call["gt_users"])
    recs = df(FX[call["recs"]])
    got = metric(recs, df(FX[call["gt"]]), k, gu) if call["gt"] else metric(recs, k, gu)
    print(call["id"], got, call["expected"])
    if isinstance(k, int):
        assert got == pytest.approx(call["expected"], **TOL)
    else:
        assert set(got) == {int(x) for x in call["expected"]}
        for kk, v in call["expected"].items():
            assert got[int(kk)] == pytest.approx(v, **TOL), kk
    if call["metric"] == "Coverage":
        want = KA["coverage_numerators"][call["id"]]
        num = metric.numerators(recs, k, gu)
        assert num == (want if isinstance(k, int) else {int(a): b for a, b in want.items()})


def _list_frame(items, user=0):
    return df([[user, it, float(len(items) - j)] for j, it in enumerate(items)])


@pytest.mark.parametrize("case", KA["by_user"], ids=[c["id"] for c in KA["by_user"]])
def test_known_answers_by_user(case):
    m, k, pred = case["metric"], case["k"], _list_frame(case["pred"])
    if m == "Unexpectedness":
        got = M.Unexpectedness(_list_frame(case["base"]))(pred, k)
    else:
        gt = df([[0, it, 1.0] for it in case["gt"]])
        if m == "NCISPrecision":       # relevance / previous relevance = the stated weight, far inside the clipping interval
            prev = df([[0, it, float(len(case["pred"]) - j) / w] for j, (it, w) in enumerate(zip(case["pred"], case["weights"]))])
            metric = M.NCISPrecision(prev, threshold=1e6)
        else:
            metric = QUALITY[m]()
        got = metric(pred, gt, k, users_df([0]))
    print(case["id"], got, case["expected"])
    assert got == pytest.approx(case["expected"], **TOL)


def _block_lists(block, extra=None):
    b = block.cpu().numpy()
    e = None if extra is None else extra.cpu().numpy()
    return [([int(x) for x in row if x >= 0], None if e is None else [float(v) for v, x in zip(e[r], row) if x >= 0])
            for r, row in enumerate(b)]


def test_enriched_recommendations_and_sorter():
    t = KA["tables"]["enriched_true_users"]
    users = torch.as_tensor(FX[t["gt_users"]], dtype=torch.int64, device=DEV)
    rec = M._columns(df(FX[t["recs"]]), torch.device(DEV), need_rel=True)
    block, _, _, _ = M.frame_to_block(M._rows_of(users, rec["user_idx"]), rec["item_idx"], rec["relevance"], len(users), t["k"])
    assert [p for p, _ in _block_lists(block)] == [r["pred"] for r in t["rows"]]
    off, items = M._gt_csr(M._columns(df(FX[t["gt"]]), torch.device(DEV)), users)
    off, items = off.cpu().numpy(), items.cpu().numpy()
    assert [sorted(items[off[r]:off[r + 1]].tolist()) for r in range(len(users))] == [sorted(r["gt"]) for r in t["rows"]]
    for name in ("sorter", "sorter_index"):
        t = KA["tables"][name]
        rows = t["rows"]
        z = torch.zeros(len(rows), dtype=torch.int32, device=DEV)
        item = torch.as_tensor([r[1] for r in rows], dtype=torch.int32, device=DEV)
        rel = torch.as_tensor([float(r[0]) for r in rows], dtype=torch.float64, device=DEV)
        pay = torch.as_tensor([float(r[2]) if len(r) > 2 else 0.0 for r in rows], dtype=torch.float64, device=DEV)
        block, _, _, w = M.frame_to_block(z, item, rel, 1, 8, payload=pay)
        (items_got, extra_got), = _block_lists(block, w)
        assert items_got == t["items"]
        if "extra" in t:
            assert extra_got == t["extra"]


def _ncis_state(metric, frame, users):
    metric(frame, frame, 8, users_df(users))
    return metric._last_block


def test_ncis_activations_clipping_and_enriched_lists():
    T = KA["tables"]
    fr = FX["prev_relevance"]
    users = sorted({r[0] for r in fr})
    for name, act in (("ncis_softmax", "softmax"), ("ncis_sigmoid", "sigmoid")):
        block, val, _ = _ncis_state(M.NCISPrecision(df(fr), activation=act), df(fr), users)
        got = {(u, it): v for u, (items, vals) in zip(users, _block_lists(block, val)) for it, v in zip(items, vals)}
        for u, it, want in T[name]["rows"]:
            print(name, u, it, got[(u, it)], want)
            assert got[(u, it)] == pytest.approx(want, **TOL)
    t = T["ncis_weigh_and_clip"]
    prev = df([[r[0], r[1], t["prev_by_user"].get(str(r[0]), t["prev_by_user"]["other"])] for r in fr])
    block, _, w = _ncis_state(M.NCISPrecision(prev, threshold=t["threshold"]), df(fr), users)
    got = {(u, it): v for u, (items, ws) in zip(users, _block_lists(block, w)) for it, v in zip(items, ws)}
    for u, it, want in t["rows"]:
        assert got[(u, it)] == pytest.approx(want, **TOL)
    t = T["ncis_enriched"]
    metric = M.NCISPrecision(df(FX[t["prev"]]))
    metric(df(FX[t["recs"]]), df(FX[t["gt"]]), t["k"])
    block, _, w = metric._last_block
    for (pred, ws), row in zip(_block_lists(block, w), t["rows"]):
        assert pred == row["pred"]
        assert ws == pytest.approx(row["weight"], **TOL)
    with pytest.raises(ValueError):
        M.NCISPrecision(df(fr), activation="absent")
    with pytest.raises(ValueError):
        M.NCISPrecision(df(fr), threshold=-1.0)


def test_relations_of_the_reference_tests():
    """test_metric_calc_with_gt_users, test_duplicate_recs, test_not_full_recs, test_user_dist, test_item_dist"""
    recs, true, dup = df(FX["recs"]), df(FX["true"]), df(FX["duplicate_recs"])
    for name, cls in QUALITY.items():
        metric = cls()
        assert metric(recs, true, 1, users_df(sorted(set(true.user_idx)))) == metric(recs, true, 1), name
        assert metric(dup, true, 4) == pytest.approx(metric(recs, true, 4), **TOL), name
        if name not in ("Precision", "MAP"):
            pred, gt = _list_frame([4, 1, 2]), df([[0, 2, 1.0], [0, 4, 1.0]])
            assert metric(pred, gt, 4) == pytest.approx(metric(pred, gt, 3), **TOL), name
    t = KA["tables"]["user_dist"]
    for name, gu in (("all", None), ("true_users", users_df(FX["true_users"]))):
        got = M.HitRate().user_distribution(df(FX[t["log"]]), recs, true, t["k"], gu).sort_values("count")
        pd.testing.assert_frame_equal(got.reset_index(drop=True), pd.DataFrame(t[name]), check_dtype=False)
    t = KA["tables"]["item_dist"]
    got = M.item_distribution(df(FX[t["log"]]), recs, t["k"])
    assert got["rec_count"].to_list() == t["rec_count"]
    want = R.item_distribution(FX[t["log"]], FX[t["recs"]], t["k"])
    assert list(zip(got.item_idx, got.user_count, got.rec_count)) == want
    with pytest.raises(ValueError):
        M.Surprisal(df(FX["one_user"]))
    with pytest.raises(ValueError):
        M.RocAuc()(df([[0, 1, float("nan")]]), true, 1)


# ---------------------------------------------------------------------------------------------------------------------
# random frames
# ---------------------------------------------------------------------------------------------------------------------
N_U, N_I, KMAX, KS = 3000, 500, 20, [1, 5, 10, 20]


def _random_frames(seed=11):
    rng = np.random.default_rng(seed)
    n_rows = rng.integers(0, 36, N_U)                  # empty users and users with more than KMAX rows
    n_rows[rng.random(N_U) < 0.05] = 0
    user = np.repeat(np.arange(N_U), n_rows)
    item = rng.integers(0, N_I + 40, len(user))        # repeats within a user happen; some items are outside the log
    grid = np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 1.5, 3.0])
    rel = np.where(rng.random(len(user)) < 0.5, grid[rng.integers(0, len(grid), len(user))], rng.normal(size=len(user)))
    p = rng.permutation(len(user))
    recs = np.stack([user[p], item[p], rel[p]], 1)
    gu = np.repeat(np.arange(N_U), rng.integers(0, 9, N_U))        # users without ground truth
    gt = np.stack([gu, rng.integers(0, N_I, len(gu)), np.ones(len(gu))], 1)
    lu = np.repeat(np.arange(N_U), rng.integers(0, 12, N_U))
    log = np.stack([lu, np.clip(rng.zipf(1.3, len(lu)) - 1, 0, N_I - 1), np.ones(len(lu))], 1)
    bu = np.repeat(np.arange(0, N_U, 2), 15)
    base = np.stack([bu, rng.integers(0, N_I, len(bu)), rng.integers(0, 6, len(bu)).astype(np.float64)], 1)
    prev = np.stack([user[::2], item[::2], rng.choice([0.0, 0.25, 1.0, 4.0, -1.0], len(user[::2]))], 1)
    return recs, gt, log, base, prev


def test_random_frames_against_the_cpu_restatement():
    recs, gt, log, base, prev = _random_frames()
    users = list(range(N_U))
    gu = users_df(users)
    dev = torch.device(DEV)
    # frame -> block and rec_pos: integers, identical
    rec = M._columns(df(recs), dev, need_rel=True)
    ut = torch.arange(N_U, device=dev, dtype=torch.int64)
    block, _, pos, _ = M.frame_to_block(M._rows_of(ut, rec["user_idx"]), rec["item_idx"], rec["relevance"], N_U, KMAX, want_pos=True)
    ref_idx, ref_pos = R.frame_to_block(recs.tolist(), users, KMAX)
    assert np.array_equal(block.cpu().numpy(), ref_idx) and np.array_equal(pos.cpu().numpy(), ref_pos)
    vec_idx, vec_pos = R.frame_to_block_np(recs[:, 0], recs[:, 1], recs[:, 2], N_U, KMAX)
    assert np.array_equal(vec_idx, ref_idx) and np.array_equal(vec_pos, ref_pos)
    raw, _, _, _ = M.frame_to_block(M._rows_of(ut, rec["user_idx"]), rec["item_idx"], rec["relevance"], N_U, KMAX, dedup=False)
    assert np.array_equal(raw.cpu().numpy(), R.frame_to_block(recs.tolist(), users, KMAX, dedup=False)[0])
    # every metric: per-user values, mean, median, confidence interval
    ctx = {"Surprisal": dict(log=log.tolist()), "Unexpectedness": dict(base=base.tolist()),
           "NCISPrecision": dict(prev=prev.tolist(), activation="softmax", threshold=3.0)}
    metrics = {n: c() for n, c in QUALITY.items()}
    metrics["Surprisal"] = M.Surprisal(df(log))
    metrics["Unexpectedness"] = M.Unexpectedness(df(base))
    metrics["NCISPrecision"] = M.NCISPrecision(df(prev), threshold=3.0, activation="softmax")
    for name, metric in metrics.items():
        rec_only = name in ("Surprisal", "Unexpectedness")
        ref_users, ref = R.per_user_values(name, recs.tolist(), KS, gt=gt.tolist(), gt_users=users, **ctx.get(name, {}))
        enr = metric._enrich(df(recs), None if rec_only else df(gt), KS, gu)
        assert enr.users.cpu().tolist() == ref_users
        got = enr.per_user.cpu().numpy()
        for q, k in enumerate(KS):
            want = np.asarray(ref[k])
            print(name, k, "max abs diff", np.abs(got[:, q] - want).max(), "mean", metric._mean(enr, k), R.mean(ref[k]))
            np.testing.assert_allclose(got[:, q], want, rtol=1e-13, atol=1e-15, err_msg=f"{name}@{k}")
            assert metric._mean(enr, k) == pytest.approx(math.fsum(ref[k]) / len(want), rel=1e-12), (name, k)
            assert metric._median(enr, k) == R.lower_median(got[:, q].tolist()), (name, k)
            assert metric._conf_interval(enr, k, 0.95) == pytest.approx(R.conf_interval(got[:, q]), rel=2.0 ** -22), (name, k)
        call = metric(df(recs), KS, gu) if rec_only else metric(df(recs), df(gt), KS, gu)
        assert call == metric._mean(enr, KS)
    # NCIS without activation and joined on the item alone
    item_prev = prev[np.unique(prev[:, 1], return_index=True)[1]]
    m2 = M.NCISPrecision(df(item_prev)[["item_idx", "relevance"]])
    _, ref = R.per_user_values("NCISPrecision", recs.tolist(), KS, gt=gt.tolist(), gt_users=users, prev=item_prev.tolist(),
                               prev_by_user=False)
    enr = m2._enrich(df(recs), df(gt), KS, gu)
    for q, k in enumerate(KS):
        np.testing.assert_allclose(enr.per_user[:, q].cpu().numpy(), np.asarray(ref[k]), rtol=1e-13, atol=1e-15)
    # default user sets (no ground_truth_users) and the rec_rows indirection
    for name in ("RocAuc", "Surprisal", "Unexpectedness"):
        metric, rec_only = metrics[name], name != "RocAuc"
        _, ref = R.per_user_values(name, recs.tolist(), KS, gt=gt.tolist(), **ctx.get(name, {}))
        got = metric(df(recs), KS) if rec_only else metric(df(recs), df(gt), KS)
        for k in KS:
            assert got[k] == pytest.approx(math.fsum(ref[k]) / len(ref[k]), rel=1e-12), (name, k)
    off, items = M._gt_csr(M._columns(df(gt), dev), ut)
    perm = torch.randperm(N_U, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    _, direct = M.evaluate_extras(block, KS, off, items)
    _, shuffled = M.evaluate_extras(block[perm].contiguous(), KS, off, items, rec_rows=perm.to(torch.int32).contiguous())
    assert torch.equal(shuffled[:, 0, :], direct[perm][:, 0, :])
    # Coverage and item_distribution: exact
    cov = M.Coverage(df(log))
    assert cov.numerators(df(recs), KS) == R.coverage_counts(recs.tolist(), KS)
    some = users[::3]
    assert cov.numerators(df(recs), KS, users_df(some)) == R.coverage_counts(recs.tolist(), KS, some)
    n_log_items = len(set(log[:, 1].tolist()))
    assert cov(df(recs), KS) == {k: c / n_log_items for k, c in R.coverage_counts(recs.tolist(), KS).items()}
    assert cov.median(df(recs), 5) == cov(df(recs), 5) and cov.conf_interval(df(recs), 5) == 0.0
    got = M.item_distribution(df(log), df(recs), 10)
    assert list(zip(got.item_idx, got.user_count, got.rec_count)) == R.item_distribution(log.tolist(), recs.tolist(), 10)
    # pyarrow and device-tensor frames give what pandas gives
    import pyarrow as pa
    tbl = pa.table({"user_idx": pa.array(recs[:, 0].astype(np.int32)), "item_idx": pa.array(recs[:, 1].astype(np.int32)),
                    "relevance": pa.array(recs[:, 2])})
    dct = {k: v for k, v in M._columns(df(recs), dev, need_rel=True).items()}
    want = metrics["RocAuc"](df(recs), df(gt), KS)
    assert metrics["RocAuc"](tbl, df(gt), KS) == want and metrics["RocAuc"](dct, df(gt), KS) == want


# ---------------------------------------------------------------------------------------------------------------------
# one large block
# ---------------------------------------------------------------------------------------------------------------------
def test_large_block_means_determinism_and_coverage():
    n, k, n_items, ks = 200_000, 10, 20_000, [1, 5, 10]
    rng = np.random.default_rng(3)
    user = np.repeat(np.arange(n), k + 2)                              # 12 rows per user, cut at 10
    item = np.clip(rng.zipf(1.2, len(user)) - 1, 0, n_items - 1)       # popular items repeat within a user
    rel = np.round(rng.normal(size=len(user)), 1)                      # ties
    p = rng.permutation(len(user))
    user, item, rel = user[p], item[p], rel[p]
    gu = np.repeat(np.arange(n), rng.integers(0, 4, n))
    gi = np.clip(rng.zipf(1.2, len(gu)) - 1, 0, n_items - 1)
    dev = torch.device(DEV)
    frame = {"user_idx": torch.as_tensor(user.astype(np.int32)).to(dev), "item_idx": torch.as_tensor(item.astype(np.int32)).to(dev),
             "relevance": torch.as_tensor(rel).to(dev)}
    gt = {"user_idx": torch.as_tensor(gu.astype(np.int32)).to(dev), "item_idx": torch.as_tensor(gi.astype(np.int32)).to(dev)}
    log = gt
    users = users_df(np.arange(n))
    ut = torch.arange(n, device=dev, dtype=torch.int64)
    block, _, pos, _ = M.frame_to_block(M._rows_of(ut, frame["user_idx"]), frame["item_idx"], frame["relevance"], n, k,
                                        want_pos=True)
    ref_idx, ref_pos = R.frame_to_block_np(user, item, rel, n, k)
    assert np.array_equal(block.cpu().numpy(), ref_idx) and np.array_equal(pos.cpu().numpy(), ref_pos)
    roc, sur, cov = M.RocAuc(), M.Surprisal(log), M.Coverage(log)
    first = (roc(frame, gt, ks, users), sur(frame, ks, users), cov.numerators(frame, ks, users))
    again = (roc(frame, gt, ks, users), sur(frame, ks, users), cov.numerators(frame, ks, users))
    assert first == again                                              # bit for bit
    off, items = M._gt_csr(gt, ut)
    cnt, n_log_users = R.item_user_counts(np.stack([gu, gi], 1).tolist())
    w = np.ones(n_items)
    for it, c in cnt.items():
        w[it] = math.log2(n_log_users / c) / math.log2(n_log_users)
    np.testing.assert_allclose(sur.item_weights.cpu().numpy(), w[:len(sur.item_weights)], rtol=1e-13, atol=1e-15)
    ref = R.block_extras_np(ref_idx, ks, off.cpu().numpy(), items.cpu().numpy(), w)
    for q, kk in enumerate(ks):
        print("large", kk, first[0][kk], first[1][kk], first[2][kk])
        assert first[0][kk] == pytest.approx(math.fsum(ref["RocAuc"][:, q]) / n, rel=1e-12)
        assert first[1][kk] == pytest.approx(math.fsum(ref["Surprisal"][:, q]) / n, rel=1e-12)
    assert first[2] == R.coverage_counts_np(ref_idx, ref_pos, ks)


# ---------------------------------------------------------------------------------------------------------------------
# CQL.evaluate(extra=...)
# ---------------------------------------------------------------------------------------------------------------------
def test_model_evaluate_extra_equals_the_classes_on_predict_output():
    from replay_cql_amd.cql import CQL
    u, i, t, r = O.synth_log(120, 700, seed=6, mean_len=14, max_len=40)
    log = pd.DataFrame({"user_idx": u, "item_idx": i, "timestamp": pd.to_datetime(t, unit="s"), "relevance": r})
    model = CQL(embedding_dim=64, window=8, batch_size=64, n_steps=12, seed=3, device=DEV)
    model.fit(log)
    test = log.sample(frac=0.15, random_state=1)[["user_idx", "item_idx"]]
    test = pd.concat([test, pd.DataFrame({"user_idx": [10_000, 10_000], "item_idx": [1, 2]})], ignore_index=True)
    train = log.drop(test.index, errors="ignore")
    ks = [1, 5, 10]
    plain = model.evaluate(train, test, ks=ks)
    assert model.evaluate(train, test, ks=ks, extra=()) == plain
    got = model.evaluate(train, test, ks=ks, extra=("RocAuc", "Coverage", "Surprisal"))
    assert {m: got[m] for m in plain} == plain and set(got) == set(plain) | {"RocAuc", "Coverage", "Surprisal"}
    recs = model.predict(train, k=10, users=test.user_idx.unique())
    gt_users = users_df(np.sort(test.user_idx.unique()))
    print(got["RocAuc"], got["Coverage"], got["Surprisal"])
    assert got["RocAuc"] == pytest.approx(M.RocAuc()(recs, test, ks), rel=1e-12, abs=1e-15)
    assert got["Surprisal"] == pytest.approx(M.Surprisal(train)(recs, ks, gt_users), rel=1e-12, abs=1e-15)
    assert got["Coverage"] == M.Coverage(model.fit_items)(recs, ks, gt_users)
    for name in M.METRICS:
        assert plain[name] == pytest.approx(getattr(M, name)()(recs, test, ks), rel=1e-12, abs=1e-15), name
    with pytest.raises(ValueError):
        model.evaluate(train, test, ks=ks, extra=("Novelty",))
