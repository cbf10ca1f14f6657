"""tests/features_reference.py, the CPU yardstick of the history-based feature processors: it reproduces every known
answer of tests/golden/history_features_known_answers.json (floats within 1e-12 -- hand-computable values -- integers,
dates and quantiles exactly), agrees with a brute-force evaluation on small random logs, follows the quantile rank rule
at the group sizes where ceil(p * n) steps, and the logs of the GPU tests have the properties those tests lean on."""
import math
import statistics

import numpy as np
import pytest

import features_reference as R

GOLDEN = R.golden()


def golden_log(case):
    return R.golden_log(GOLDEN, case)


def check_rows(fit, pre, columns, rows, id_map):
    cols = fit[pre]["cols"]
    for row in rows:
        g = id_map[row[0]]
        assert fit[pre]["count"][g] > 0
        for name, want in zip(columns[1:], row[1:]):
            got = cols[name][g]
            if name.endswith("_interact_date"):
                assert got == np.datetime64(want, "ns").astype(np.int64), (name, row)
            elif isinstance(want, int) or "quantile" in name:
                assert got == want, (name, row)
            else:
                assert abs(got - want) <= 1e-12, (name, row, got)


def test_no_ts_rel_known_answers():
    case = GOLDEN["cases"]["no_ts_rel"]
    fit = R.fit_reference(golden_log("no_ts_rel"))
    assert not fit["calc_relevance_based"] and not fit["calc_timestamp_based"]
    assert sorted(R.feature_names(fit, "u")) == sorted(GOLDEN["column_groups"]["simple_u"])
    assert sorted(R.feature_names(fit, "i")) == sorted(GOLDEN["column_groups"]["simple_i"])
    check_rows(fit, "u", case["user_columns"], case["user_rows"], GOLDEN["ids"]["user"])
    check_rows(fit, "i", case["item_columns"], case["item_rows"], GOLDEN["ids"]["item"])


def test_ts_no_rel_known_answers():
    case, groups = GOLDEN["cases"]["ts_no_rel"], GOLDEN["column_groups"]
    fit = R.fit_reference(golden_log("ts_no_rel"))
    assert not fit["calc_relevance_based"] and fit["calc_timestamp_based"]
    assert sorted(R.feature_names(fit, "u")) == sorted(groups["simple_u"] + ["u_" + c for c in groups["time"]])
    assert sorted(R.feature_names(fit, "i")) == sorted(groups["simple_i"] + ["i_" + c for c in groups["time"]])
    check_rows(fit, "u", case["user_columns"], case["user_rows"], GOLDEN["ids"]["user"])


def test_relevance_ts_known_answers():
    case, groups = GOLDEN["cases"]["relevance_ts"], GOLDEN["column_groups"]
    fit = R.fit_reference(golden_log("relevance_ts"))
    assert fit["calc_relevance_based"] and fit["calc_timestamp_based"] and fit["has_cr"]
    assert sorted(R.feature_names(fit, "u")) == sorted(
        groups["simple_u"] + ["u_" + c for c in groups["time"] + groups["relevance"]] + groups["abnormality"])
    assert sorted(R.feature_names(fit, "i")) == sorted(
        groups["simple_i"] + ["i_" + c for c in groups["time"] + groups["relevance"]])
    check_rows(fit, "i", case["item_columns"], case["item_rows"], GOLDEN["ids"]["item"])
    check_rows(fit, "u", case["user_columns"], case["user_rows"], GOLDEN["ids"]["user"])


def test_conditional_popularity_known_answers():
    ids, case = GOLDEN["ids"], GOLDEN["cases"]["conditional_features"]
    log = golden_log("relevance_ts")
    gender = {ids["user"][r[0]]: r[3] for r in GOLDEN["user_features"]["rows"]}
    table = R.conditional_popularity(log["item_idx"], log["user_idx"], gender)
    want = {(ids["item"][r[0]], r[1]): r[2] for r in case["rows"]}
    got = {(e, c): p for e, c, p in table if e in (ids["item"]["i1"], ids["item"]["i2"])}
    assert got == want
    share, na = R.popularity_lookup(table, [0, 0, 1, 2], ["M", "X", None, "F"])
    assert share.tolist() == [0.5, 0.0, 0.0, 0.5] and na.tolist() == [False, True, True, False]


@pytest.mark.parametrize("n", R.QUANTILE_SIZES)
def test_quantile_rank_rule(n):
    """the element at 1-based rank clamp(ceil(p * n), 1, n): where p * n is integral the rank is that integer, otherwise
    the next one; the listed sizes are those around the steps of ceil(0.05 n) and ceil(0.95 n)"""
    want = {1: (1, 1, 1), 2: (1, 1, 2), 19: (1, 10, 19), 20: (1, 10, 19), 21: (2, 11, 20), 39: (2, 20, 38),
            40: (2, 20, 38), 41: (3, 21, 39), 100: (5, 50, 95)}[n]
    assert tuple(R.quantile_rank(p, n) for _, p in R.QUANTILES) == want
    x = np.arange(n, dtype=np.float64) * 0.5 + 0.5
    user = np.append(np.zeros(n, dtype=np.int64), 1)              # a second user keeps relevance from being constant
    fit = R.log_stat_features(user, np.arange(n + 1) % 3, np.append(x[::-1], 99.0))
    for (name, _), rank in zip(R.QUANTILES, want):
        assert fit["u"]["cols"]["u_" + name][0] == x[rank - 1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_agrees_with_brute_force_on_small_random_logs(seed):
    rng = np.random.default_rng(seed)
    n = 60
    user, item = rng.integers(0, 9, n), rng.integers(0, 7, n)
    rel = rng.integers(1, 11, n) * 0.5
    ts = rng.integers(-3 * R.DAY_S, 5 * R.DAY_S, n)
    fit = R.log_stat_features(user, item, rel, ts)
    assert fit["calc_relevance_based"] and fit["calc_timestamp_based"]
    rows_of = {"u": lambda g: [k for k in range(n) if user[k] == g], "i": lambda g: [k for k in range(n) if item[k] == g]}
    stats = {}
    for pre, n_groups in (("u", int(user.max()) + 1), ("i", int(item.max()) + 1)):
        for g in range(n_groups):
            rows, cols = rows_of[pre](g), fit[pre]["cols"]
            assert fit[pre]["count"][g] == len(rows)
            if not rows:
                assert all(cols[c][g] == 0 for c in R.feature_names(fit, pre, False))
                continue
            x = sorted(float(rel[k]) for k in rows)
            days = sorted({int(ts[k]) // R.DAY_S for k in rows})              # Python's // floors
            stats[pre, g] = (math.fsum(x) / len(x), statistics.stdev(x) if len(x) > 1 else 0.0)
            assert abs(cols[pre + "_log_num_interact"][g] - math.log(len(rows))) <= 1e-15
            assert cols[pre + "_distinct_days"][g] == len(days)
            assert cols[pre + "_min_interact_date"][g] == min(int(ts[k]) for k in rows)
            assert cols[pre + "_history_length_days"][g] == max(int(ts[k]) for k in rows) // R.DAY_S - days[0]
            assert cols[pre + "_last_interaction_gap_days"][g] == int(ts.max()) // R.DAY_S - days[-1]
            assert cols[pre + "_mean"][g] == stats[pre, g][0]
            assert abs(cols[pre + "_std"][g] - stats[pre, g][1]) <= 1e-14
            for name, p in R.QUANTILES:
                assert cols[pre + "_" + name][g] == x[max(1, min(len(x), math.ceil(p * len(x)))) - 1]
    stds = [stats["i", g][1] for g in range(int(item.max()) + 1) if ("i", g) in stats]
    lo, hi = min(stds), max(stds)
    for g in range(int(user.max()) + 1):
        rows = rows_of["u"](g)
        if not rows:
            continue
        ab = [abs(float(rel[k]) - stats["i", int(item[k])][0]) for k in rows]
        cr = [(a * (1 - (stats["i", int(item[k])][1] - lo) / (hi - lo))) ** 2 for a, k in zip(ab, rows)]
        cross = [math.log(sum(1 for j in range(n) if item[j] == item[k])) for k in rows]
        cols = fit["u"]["cols"]
        assert abs(cols["abnormality"][g] - math.fsum(ab) / len(ab)) <= 1e-14
        assert abs(cols["abnormalityCR"][g] - math.fsum(cr) / len(cr)) <= 1e-13
        assert abs(cols["u_mean_i_log_num_interact"][g] - math.fsum(cross) / len(cross)) <= 1e-14


def test_transform_is_a_left_join_with_zero_fill_then_the_differences():
    fit = R.fit_reference(golden_log("relevance_ts"))
    out = R.transform(fit, [0, 7, 2, -1], [3, 1, 9, 0])
    assert list(out) == R.block_names(fit)
    assert out["na_u_log_features"].tolist() == [0, 1, 0, 1] and out["na_i_log_features"].tolist() == [0, 0, 1, 0]
    assert out["u_mean"][1] == 0 and out["i_std"][2] == 0
    u_log, i_cross = fit["u"]["cols"]["u_log_num_interact"], fit["i"]["cols"]["i_mean_u_log_num_interact"]
    assert out["u_i_log_num_interact_diff"].tolist() == [u_log[0] - i_cross[3], 0 - i_cross[1], u_log[2] - 0, 0 - i_cross[0]]


def test_the_logs_of_the_gpu_tests_have_the_properties_they_are_built_for():
    log = R.ties_log()
    n = len(log["user_idx"])
    assert n == 20000 and log["user_idx"].max() == 320 and len(np.unique(log["user_idx"])) == 300
    items = np.bincount(log["item_idx"], minlength=97)
    assert len(items) == 97 and items[0] > 5000 and items[90:95].tolist() == [1, 1, 1, 2, 2] and (items > 0).all()
    users = np.bincount(log["user_idx"])
    assert users.max() == 4097 and (users == 1).sum() >= 3 and (users == 0).sum() == 21
    assert (log["timestamp"] < 0).any() and (log["timestamp"] % R.DAY_S == 0).sum() > n // 5
    assert len(np.unique(log["timestamp"] // R.DAY_S)) == 40
    assert set(np.unique(log["relevance"] * 2)) == set(range(1, 11))
    for offset in (0.0, 2.0 ** 20):
        fit = R.fit_reference(R.ties_log(offset))
        std = np.sort(fit["i"]["cols"]["i_std"][fit["i"]["count"] > 0])
        assert fit["has_cr"] and std[-1] - std[0] > 1.0          # far from flipping the abnormalityCR branch on rounding
        # the sum of squares of the naive variance formula loses the variance altogether at this offset
        if offset:
            x = R.ties_log(offset)["relevance"][log["item_idx"] == 0]
            naive = (np.sum(x * x) - np.sum(x) ** 2 / len(x)) / (len(x) - 1)
            assert abs(math.sqrt(max(naive, 0.0)) - fit["i"]["cols"]["i_std"][0]) > 1e-6
    sized, sizes = R.sizes_log()
    assert np.bincount(sized["user_idx"]).tolist() == sizes
    assert all(len(np.unique(sized["relevance"][sized["user_idx"] == g])) == s for g, s in enumerate(sizes))
