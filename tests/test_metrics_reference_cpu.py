"""CPU side of the extended metrics: tests/metrics_reference.py reproduces every known answer of the reference's metric
tests (tests/golden/metrics_known_answers.json), and every new C entry point validates its arguments on the host, before
any HIP call."""
import ctypes as C
import json
from pathlib import Path

import pytest

from replay_cql_amd import _native as N
from replay_cql_amd import build as B
from tests import metrics_reference as R

KA = json.loads((Path(__file__).resolve().parent / "golden" / "metrics_known_answers.json").read_text())
FX = KA["fixtures"]
TOL = dict(rel=1e-12, abs=1e-15)


def _ctx(call):
    m, init = call["metric"], call["init"]
    return {"log": FX[init] if m == "Surprisal" else None, "base": FX[init] if m == "Unexpectedness" else None}


def _gt_users(spec):
    return FX[spec] if isinstance(spec, str) else spec


@pytest.mark.parametrize("call", KA["calls"], ids=[c["id"] for c in KA["calls"]])
def test_known_answers_of_whole_calls(call):
    ks = [call["k"]] if isinstance(call["k"], int) else call["k"]
    frame, gt_users = FX[call["recs"]], _gt_users(call["gt_users"])
    if call["metric"] == "Coverage":
        counts = R.coverage_counts(frame, ks, gt_users)
        n_items = len({r[1] for r in FX[call["init"]]})
        got = {k: counts[k] / n_items for k in ks}
        want_n = KA["coverage_numerators"][call["id"]]
        assert counts == ({int(k): v for k, v in want_n.items()} if isinstance(want_n, dict) else {ks[0]: want_n})
    else:
        _, vals = R.per_user_values(call["metric"], frame, ks, gt=FX[call["gt"]] if call["gt"] else None,
                                    gt_users=gt_users, **_ctx(call))
        got = {k: R.mean(vals[k]) for k in ks}
    want = call["expected"]
    if isinstance(call["k"], int):
        assert got[call["k"]] == pytest.approx(want, **TOL)
    else:
        assert set(got) == {int(k) for k in want}
        for k, v in want.items():
            assert got[int(k)] == pytest.approx(v, **TOL), k


@pytest.mark.parametrize("case", KA["by_user"], ids=[c["id"] for c in KA["by_user"]])
def test_known_answers_by_user(case):
    m, k = case["metric"], case["k"]
    if m == "Unexpectedness":
        got = R.unexpectedness(k, case["pred"], case["base"])
    elif m == "NCISPrecision":
        got = R.ncis_precision(k, case["pred"], case["gt"], case["weights"])
    else:
        got = R.quality_by_user(m, k, case["pred"], case["gt"])
    assert got == pytest.approx(case["expected"], **TOL)


def test_enriched_recommendations_with_ground_truth_users():
    t = KA["tables"]["enriched_true_users"]
    lists, gts = R.user_lists(FX[t["recs"]], t["k"]), R.gt_sets(FX[t["gt"]])
    assert [r["user"] for r in t["rows"]] == FX[t["gt_users"]]
    for row in t["rows"]:
        assert lists.get(row["user"], ([],))[0] == row["pred"]
        assert sorted(gts.get(row["user"], ())) == sorted(row["gt"])


def test_sorter():
    t = KA["tables"]["sorter"]
    assert R.user_lists([(0, i, r) for r, i in t["rows"]], 100)[0][0] == t["items"]
    t = KA["tables"]["sorter_index"]
    items, _, _, extra = R.user_lists([(0, i, r) for r, i, _ in t["rows"]], 100, payload=[x for _, _, x in t["rows"]])[0]
    assert items == t["items"] and extra == t["extra"]


def test_ncis_activations_and_clipping():
    T = KA["tables"]
    fr = FX["prev_relevance"]
    users, rel = [r[0] for r in fr], [r[2] for r in fr]
    for got, want in zip(R.softmax_by_user(users, rel), T["ncis_softmax"]["rows"]):
        assert got == pytest.approx(want[2], **TOL)
    for got, want in zip(R.sigmoid(rel), T["ncis_sigmoid"]["rows"]):
        assert got == pytest.approx(want[2], **TOL)
    t = T["ncis_weigh_and_clip"]
    prev = [t["prev_by_user"].get(str(u), t["prev_by_user"]["other"]) for u in users]
    for got, want in zip(R.weigh_and_clip(rel, prev, t["threshold"]), t["rows"]):
        assert got == pytest.approx(want[2], **TOL)


def test_ncis_enriched_recommendations():
    t = KA["tables"]["ncis_enriched"]
    lists = R.ncis_lists(FX[t["recs"]], FX[t["prev"]], t["k"])
    for row in t["rows"]:
        pred, w = lists[row["user"]]
        assert pred == row["pred"]
        assert w == pytest.approx(row["weight"], **TOL)


def test_relations_of_the_reference_tests():
    """test_metric_calc_with_gt_users, test_not_full_recs, test_duplicate_recs, test_user_dist, test_item_dist"""
    gt_users = sorted({r[0] for r in FX["true"]})
    for m in KA["quality_metrics"]:
        a = R.per_user_values(m, FX["recs"], [1], gt=FX["true"], gt_users=gt_users)[1][1]
        b = R.per_user_values(m, FX["recs"], [1], gt=FX["true"])[1][1]
        assert R.mean(a) == R.mean(b), m
        if m not in ("Precision", "MAP"):
            assert R.quality_by_user(m, 4, [4, 1, 2], [2, 4]) == pytest.approx(R.quality_by_user(m, 3, [4, 1, 2], [2, 4]), **TOL)
        a = R.per_user_values(m, FX["duplicate_recs"], [4], gt=FX["true"])[1][4]
        b = R.per_user_values(m, FX["recs"], [4], gt=FX["true"])[1][4]
        assert R.mean(a) == pytest.approx(R.mean(b), **TOL), m
    t = KA["tables"]["user_dist"]
    for name, gu in (("all", None), ("true_users", FX["true_users"])):
        users, vals = R.per_user_values(t["metric"], FX[t["recs"]], [t["k"]], gt=FX[t["gt"]], gt_users=gu)
        dist = R.user_distribution(users, vals[t["k"]], FX[t["log"]])
        assert [c for c, _ in dist] == t[name]["count"]
        assert [v for _, v in dist] == pytest.approx(t[name]["value"], **TOL)
    t = KA["tables"]["item_dist"]
    assert [r[2] for r in R.item_distribution(FX[t["log"]], FX[t["recs"]], t["k"])] == t["rec_count"]


def test_surprisal_of_a_single_user_log_is_refused():
    with pytest.raises(ValueError):
        R.surprisal_weights(FX["one_user"])


# ---------------------------------------------------------------------------------------------------------------------
# host-side validation of the new entry points (no GPU: every check comes before the first HIP call)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def _buf(n=64):
    b = (C.c_double * n)()
    return b, C.addressof(b)


def test_new_entry_points_validate_on_the_host(lib):
    keep, p = _buf(4096)
    ks = lambda *v: (C.c_int32 * len(v))(*v)           # noqa: E731
    big = 1 << 40

    def bad(match, rc):
        with pytest.raises(N.CqlrecError, match=match):
            N.check(rc)

    # frame -> block
    assert lib.cqlrec_recs_frame_to_block_ws_bytes(1000, 10) > 2 * 1000 * 4 + 2 * 1000 * 8
    bad("NULL", lib.cqlrec_recs_frame_to_block(None, None, None, None, 8, 4, 2, 1, p, big, p, None, None, None, None))
    bad("NULL", lib.cqlrec_recs_frame_to_block(p, p, p, None, 8, 4, 2, 1, None, big, p, None, None, None, None))
    bad("go together", lib.cqlrec_recs_frame_to_block(p, p, p, p, 8, 4, 2, 1, p, big, p, None, None, None, None))
    bad("kmax", lib.cqlrec_recs_frame_to_block(p, p, p, None, 8, 4, 0, 1, p, big, p, None, None, None, None))
    bad("workspace too small", lib.cqlrec_recs_frame_to_block(p, p, p, None, 8, 4, 2, 1, p, 16, p, None, None, None, None))
    # join, NCIS weights
    bad("NULL", lib.cqlrec_recs_join_prev(None, None, 3, None, p, 8, p, None))
    bad("NULL", lib.cqlrec_recs_join_prev(p, p, 3, None, None, 8, p, None))
    bad("NULL", lib.cqlrec_recs_ncis_weights(p, None, p, 4, 2, 0, 10.0, None))
    bad("activation", lib.cqlrec_recs_ncis_weights(p, p, p, 4, 2, 7, 10.0, None))
    bad("threshold", lib.cqlrec_recs_ncis_weights(p, p, p, 4, 2, 0, 0.0, None))
    # per-user extras
    assert lib.cqlrec_eval_extras_ws_bytes(1000, 3) >= 4 * 4 * 3 * 8
    ex = lambda **kw: lib.cqlrec_eval_extras(  # noqa: E731
        kw.get("rec", p), 4, 5, None, p, p, None, 0, None, 0, None, kw.get("ks", ks(1, 3)), kw.get("n_ks", 2),
        kw.get("ws", p), kw.get("wsb", big), None, kw.get("sums", p), None)
    bad("NULL", ex(rec=None))
    bad("NULL", ex(sums=None))
    bad("NULL", ex(ws=None))
    bad("ascending", ex(ks=ks(3, 1)))
    bad("ascending", ex(ks=ks(1, 6)))
    bad("out of range", ex(ks=ks(*range(1, 10)), n_ks=9))
    bad("workspace too small", ex(wsb=8))
    bad("go together", lib.cqlrec_eval_extras(p, 4, 5, None, p, None, None, 0, None, 0, None, ks(1), 1, p, big, None, p, None))
    # item side
    assert lib.cqlrec_eval_item_user_counts_ws_bytes(1000) > 2 * 1000 * 8
    bad("NULL", lib.cqlrec_eval_item_user_counts(None, p, 8, 4, p, big, p, p, None))
    bad("workspace too small", lib.cqlrec_eval_item_user_counts(p, p, 8, 4, p, 8, p, p, None))
    bad("NULL", lib.cqlrec_eval_surprisal_weights(None, 4, 3, p, None))
    bad("n_users", lib.cqlrec_eval_surprisal_weights(p, 4, 1, p, None))
    bad("NULL", lib.cqlrec_eval_coverage(p, None, 4, 5, 6, ks(1), 1, p, p, None))
    bad("ascending", lib.cqlrec_eval_coverage(p, p, 4, 5, 6, ks(3, 3), 2, p, p, None))
    bad("out of range", lib.cqlrec_eval_coverage(p, p, 4, 5, 6, ks(*range(1, 10)), 9, p, p, None))
    bad("NULL", lib.cqlrec_eval_item_hist(None, 4, 5, 6, p, None))
    bad("n_items", lib.cqlrec_eval_item_hist(p, 4, 5, 0, p, None))
    del keep


def test_metric_classes_validate_before_touching_the_gpu():
    from replay_cql_amd import metrics as M
    with pytest.raises(ValueError, match="activation"):
        M.NCISPrecision(prev_policy_weights=None, activation="absent")
    with pytest.raises(ValueError, match="[Tt]hreshold"):
        M.NCISPrecision(prev_policy_weights=None, threshold=0.0)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(N.CqlrecError, match="no CPU path"):
            M.RocAuc()([[0, 0, 1.0]], [[0, 0, 1.0]], 1)
