"""tests/filter_reference.py, the numpy yardstick of the GPU filters, against the known answers of
tests/golden/filters_known_answers.json and against brute force on small random logs with many ties."""
import json
from pathlib import Path

import numpy as np
import pytest

import filter_reference as F

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "filters_known_answers.json").read_text())


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_reference_reproduces_the_known_answers(case):
    got = F.keep_rows(case["filter"], F.golden_args(case["args"]), F.golden_log(case["log"]))
    assert got.dtype == np.int64 and got.tolist() == case["kept_rows"]


def test_golden_file_is_data_with_a_note_and_sources():
    assert GOLDEN["note"] and "item_col=None" in GOLDEN["note"]
    assert all(c["source"] and c["note"] and c["name"] for c in GOLDEN["cases"]) and len(GOLDEN["cases"]) == 9
    assert GOLDEN["indexer"]["source"] and GOLDEN["indexer"]["note"]


def test_dict_indexer_on_the_known_answer_and_on_unseen_ids():
    g = GOLDEN["indexer"]
    ix = F.DictIndexer()
    ix.fit(g["frame"]["user_idx"], g["frame"]["item_idx"])
    assert ix.transform("user", g["frame"]["user_idx"]).tolist() == g["transformed"]["user_idx"]
    assert ix.transform("item", g["frame"]["item_idx"]).tolist() == g["transformed"]["item_idx"]
    assert ix.inverse_transform("user", [0]).tolist() == g["frame"]["user_idx"]
    ix.fit([7, -3, 7, 10 ** 12], [1])
    assert ix.labels["user"] == [-3, 7, 10 ** 12]
    assert ix.transform("user", [7, 99, -50, 7, 99]).tolist() == [1, 4, 3, 1, 4]         # appended ascending: -50, 99
    assert ix.labels["user"] == [-3, 7, 10 ** 12, -50, 99]
    with pytest.raises(ValueError):
        ix.inverse_transform("user", [5])


def small_log(seed, n=60, ts_kind="int"):
    rng = np.random.default_rng(seed)
    user = rng.integers(0, 6, n)
    item = rng.integers(0, 4, n)
    day = rng.integers(0, 5, n)
    if ts_kind == "int":
        ts = (day * 43200).astype(np.int64)                      # half days: values on and between day bounds
    elif ts_kind == "float":
        ts = (day - 2).astype(np.float64) * 43200.5
    else:
        ts = (1577836800 + day * 43200).astype("datetime64[s]").astype("datetime64[ns]")
    return {"user_idx": user.astype(np.int64), "item_idx": item.astype(np.int64),
            "relevance": rng.choice(np.array([0.0, 1.0, 2.5, np.nan]), n), "timestamp": ts}


def brute_take(log, k, first, with_item):
    """per user, a Python sort of (timestamp, item, row) tuples"""
    keep = []
    for u in set(log["user_idx"].tolist()):
        rows = [i for i in range(len(log["user_idx"])) if log["user_idx"][i] == u]
        rows.sort(key=lambda i: (log["timestamp"][i], log["item_idx"][i] if with_item else 0, i))
        if not first:
            rows.reverse()
        keep += rows[:max(k, 0)]
    return sorted(keep)


@pytest.mark.parametrize("ts_kind", ["int", "float", "datetime"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rank_filter_against_per_user_sorting(seed, ts_kind):
    log = small_log(seed, ts_kind=ts_kind)
    for k in (-1, 0, 1, 2, 5, 100):
        for first in (True, False):
            for item_col in ("item_idx", None):
                got = F.keep_rows("take_num_user_interactions",
                                  dict(num_interactions=k, first=first, item_col=item_col), log)
                assert got.tolist() == brute_take(log, k, first, item_col is not None), (k, first, item_col)


@pytest.mark.parametrize("seed", [3, 4])
def test_first_n_and_last_c_minus_n_partition_every_user(seed):
    log = small_log(seed, n=90)
    user = log["user_idx"]
    counts = np.bincount(user)
    for item_col in ("item_idx", None):
        for n in range(0, int(counts.max()) + 1):
            head = F.keep_mask("take_num_user_interactions", dict(num_interactions=n, item_col=item_col), log)
            for u in np.flatnonzero(counts >= n):
                tail = F.keep_mask("take_num_user_interactions",
                                   dict(num_interactions=int(counts[u]) - n, first=False, item_col=item_col), log)
                mine = user == u
                assert not (head & tail & mine).any() and ((head | tail) & mine).sum() == counts[u]


@pytest.mark.parametrize("ts_kind", ["int", "float", "datetime"])
def test_day_filters_against_brute_force(ts_kind):
    log = small_log(5, ts_kind=ts_kind)
    ts = log["timestamp"]
    sec = ts.astype("datetime64[ns]").astype(np.int64) / 1e9 if ts_kind == "datetime" else ts.astype(np.float64)
    for days in (0, 1, 2, 10 ** 6):
        for first in (True, False):
            want_user, want_global = [], []
            for i in range(len(sec)):
                mine = sec[log["user_idx"] == log["user_idx"][i]]
                want_user.append(sec[i] < mine.min() + 86400 * days if first else sec[i] > mine.max() - 86400 * days)
                want_global.append(sec[i] < sec.min() + 86400 * days if first else sec[i] > sec.max() - 86400 * days)
            assert F.keep_mask("take_num_days_of_user_hist", dict(days=days, first=first), log).tolist() == want_user
            assert F.keep_mask("take_num_days_of_global_hist", dict(duration_days=days, first=first),
                               log).tolist() == want_global
    for bad in (1.0, 1.5, True, "1"):
        with pytest.raises(ValueError):
            F.keep_mask("take_num_days_of_user_hist", dict(days=bad), log)


def test_monotone_in_num_entries_and_days():
    log = small_log(6, n=120)
    for group_by in ("user_idx", "item_idx"):
        masks = [F.keep_mask("filter_by_min_count", dict(num_entries=k, group_by=group_by), log) for k in range(0, 40)]
        assert masks[0].all() and masks[1].all() and not masks[-1].any()
        assert all((b <= a).all() for a, b in zip(masks, masks[1:]))                 # a larger threshold keeps a subset
        counts = np.bincount(log[group_by])
        assert all((m == (counts[log[group_by]] >= k)).all() for k, m in enumerate(masks))
    for name, arg in (("take_num_days_of_user_hist", "days"), ("take_num_days_of_global_hist", "duration_days")):
        for first in (True, False):
            masks = [F.keep_mask(name, {arg: d, "first": first}, log) for d in (-1, 0, 1, 2, 3, 10)]
            assert not masks[0].any() and not masks[1].any() and masks[-1].all()
            assert all((a <= b).all() for a, b in zip(masks, masks[1:]))             # more days keep a superset


def test_low_ratings_drop_nan_and_keep_the_threshold_itself():
    log = {"relevance": np.array([np.nan, -0.0, 0.0, 2.5, 2.4999999999999996, np.inf, -np.inf])}
    assert F.keep_rows("filter_out_low_ratings", dict(value=2.5), log).tolist() == [3, 5]
    assert F.keep_rows("filter_out_low_ratings", dict(value=0.0), log).tolist() == [1, 2, 3, 4, 5]
    assert F.keep_rows("filter_out_low_ratings", dict(value=float("nan")), log).tolist() == []


def test_int64_bounds_saturate():
    top, low = (1 << 63) - 1, -(1 << 63)
    log = {"user_idx": np.array([0, 0, 1, 1]), "timestamp": np.array([top - 5, top, low, low + 5], dtype=np.int64)}
    # user 0: min + span saturates at the top, and ts < INT64_MAX keeps every row but the one AT the limit;
    # user 1: max - span saturates at the bottom likewise (days = 10^13: the span itself still fits)
    assert F.keep_rows("take_num_days_of_user_hist", dict(days=10 ** 13), log).tolist() == [0, 2, 3]
    assert F.keep_rows("take_num_days_of_user_hist", dict(days=10 ** 13, first=False), log).tolist() == [0, 1, 3]
    # the span saturates first (at INT64_MAX), then the add: INT64_MIN + INT64_MAX = -1, INT64_MAX - INT64_MAX = 0
    assert F.keep_rows("take_num_days_of_global_hist", dict(duration_days=10 ** 18), log).tolist() == [2, 3]
    assert F.keep_rows("take_num_days_of_global_hist", dict(duration_days=10 ** 18, first=False), log).tolist() == [0, 1]
    assert F.keep_rows("take_num_days_of_user_hist", dict(days=10 ** 30), log).tolist() == [0, 2, 3]
    assert F.keep_rows("take_num_days_of_user_hist", dict(days=10 ** 30, first=False), log).tolist() == [0, 1, 3]
    assert F.keep_rows("take_num_days_of_user_hist", dict(days=-10 ** 30), log).tolist() == []


def test_time_period_bounds():
    log = small_log(7, ts_kind="datetime")
    ts = log["timestamp"]
    every = np.arange(len(ts)).tolist()
    assert F.keep_rows("take_time_period", {}, log).tolist() == every
    edge = "2020-01-02 00:00:00"                                    # an existing timestamp: day index 2
    at = np.datetime64("2020-01-02T00:00:00")
    assert (ts == at).any()
    assert F.keep_rows("take_time_period", dict(start_date=edge), log).tolist() == np.flatnonzero(ts >= at).tolist()
    assert F.keep_rows("take_time_period", dict(end_date=edge), log).tolist() == np.flatnonzero(ts < at).tolist()
    assert F.keep_rows("take_time_period", dict(start_date=edge, end_date=edge), log).tolist() == []
    assert F.keep_rows("take_time_period", dict(start_date=1577923200, end_date="2020-01-02 00:00:01"),
                       log).tolist() == np.flatnonzero(ts == at).tolist()
