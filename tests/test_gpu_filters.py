"""The filters and the Indexer on the GPU (replay_cql_amd.filters / .indexer, csrc/prepare.hip) against
tests/filter_reference.py: the device result is the reference's EXACTLY -- the same ascending int64 row indices, the same
int32 indices -- since this is integer work (and the two double expressions are single IEEE operations on both sides).

The log of most tests is split_reference.edge_log(): 70 001 rows (no multiple of a block, many blocks), 3 000 user slots
some of which have no rows, one user of 5 000 rows, users of 1 and 2 rows, 50 distinct timestamps (ties everywhere)."""
import json
import logging
from datetime import datetime
from pathlib import Path

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

import filter_reference as R
import split_reference as SR
from replay_cql_amd import data as D
from replay_cql_amd import filters as F
from replay_cql_amd import splitters as S
from replay_cql_amd.indexer import Indexer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "filters_known_answers.json").read_text())
KINDS = ["int", "float", "datetime"]
_LOGS, _DEVICE_LOGS = {}, {}


def edge(ts_kind="int"):
    """edge_log with a relevance column that holds NaN, -0.0 and +0.0 besides its five values"""
    if ts_kind not in _LOGS:
        log = SR.edge_log(ts_kind=ts_kind)
        rel = log["relevance"].copy()
        rel[::7] = np.nan
        rel[1::11] = -0.0
        _LOGS[ts_kind] = dict(log, relevance=rel)
    return _LOGS[ts_kind]


def half_days(ts_kind):
    """edge_log with its 50 distinct timestamps half a day apart: every second one is exactly on a bound `extreme +
    k days`, the others lie between two bounds; the float ones are negative and, off the bounds, fractional"""
    key = "half_" + ts_kind
    if key not in _LOGS:
        log = SR.edge_log(ts_kind="int")
        day = (log["timestamp"] - SR.DAY0) // 86400
        if ts_kind == "int":
            ts = (SR.DAY0 + day * 43200).astype(np.int64)
        elif ts_kind == "float":
            ts = (day - 60).astype(np.float64) * 43200.0 + (day % 2) * 0.25
        else:
            ts = (SR.DAY0 + day * 43200).astype("datetime64[s]").astype("datetime64[ns]")
        _LOGS[key] = dict(log, timestamp=ts)
    return _LOGS[key]


def on_device(log, key=None):
    if key is not None and key in _DEVICE_LOGS:
        return _DEVICE_LOGS[key]
    out = {k: torch.as_tensor(v).to(DEV) for k, v in log.items()}
    if key is not None:
        _DEVICE_LOGS[key] = out
    return out


def given(log, ts_kind, key=None):
    """datetime64 has no torch dtype: those logs go in as pandas, the others as device tensors"""
    return pd.DataFrame(log) if ts_kind == "datetime" else on_device(log, key)


def check(name, args, log, device_log):
    want = R.keep_rows(name, args, log)
    got = getattr(F, name)(device_log, **args, return_rows=True)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1
    got = got.cpu().numpy()
    print(name, args, "kept", len(got), "of", len(next(iter(log.values()))))
    assert np.array_equal(got, want), (name, args)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# every filter over its parameter grid, on the edge log
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("item_col", ["item_idx", None])
@pytest.mark.parametrize("num_interactions", [0, 1, 2, 7, 5000, 10 ** 6])
def test_take_num_user_interactions_grid(num_interactions, item_col, first):
    log = edge()
    got = check("take_num_user_interactions", dict(num_interactions=num_interactions, first=first, item_col=item_col), log,
                on_device(log, "int"))
    counts = np.bincount(log["user_idx"])
    assert len(got) == np.minimum(counts, num_interactions).sum()


@pytest.mark.parametrize("ts_kind", KINDS)
def test_take_num_user_interactions_timestamp_dtypes_and_the_partition(ts_kind):
    log = edge(ts_kind)
    dev = given(log, ts_kind, ts_kind)
    if ts_kind == "float":
        assert (log["timestamp"] < 0).any() and (log["timestamp"] != np.round(log["timestamp"])).any()
    for item_col in ("item_idx", None):
        for first in (True, False):
            check("take_num_user_interactions", dict(num_interactions=3, first=first, item_col=item_col), log, dev)
    # for a user of c rows, (first=True, n) and (first=False, c - n) partition the user's rows: the user of 5 000 rows
    user, c, n = log["user_idx"], 5000, 1234
    mine = np.flatnonzero(user == 7)
    assert len(mine) == c
    for item_col in ("item_idx", None):
        head = check("take_num_user_interactions", dict(num_interactions=n, item_col=item_col), log, dev)
        tail = check("take_num_user_interactions", dict(num_interactions=c - n, first=False, item_col=item_col), log, dev)
        head, tail = np.intersect1d(head, mine), np.intersect1d(tail, mine)
        assert len(head) == n and len(tail) == c - n and len(np.intersect1d(head, tail)) == 0
        assert np.array_equal(np.union1d(head, tail), mine)
    # the tie rule: with the item left out, the LAST row of a user is the later input row among its latest timestamp
    last = check("take_num_user_interactions", dict(num_interactions=1, first=False, item_col=None), log, dev)
    t = log["timestamp"]
    assert np.intersect1d(last, mine).tolist() == [mine[t[mine] == t[mine].max()].max()]
    first_rows = check("take_num_user_interactions", dict(num_interactions=1, item_col=None), log, dev)
    assert np.intersect1d(first_rows, mine).tolist() == [mine[t[mine] == t[mine].min()].min()]


@pytest.mark.parametrize("group_by", ["user_idx", "item_idx"])
@pytest.mark.parametrize("num_entries", [1, 2, 3, 50, 5001])
def test_filter_by_min_count_grid(num_entries, group_by):
    log = edge()
    got = check("filter_by_min_count", dict(num_entries=num_entries, group_by=group_by), log, on_device(log, "int"))
    if num_entries == 1:
        assert len(got) == len(log["user_idx"])
    if num_entries == 5001:
        assert len(got) == 0
    if num_entries == 3 and group_by == "user_idx":
        assert not np.isin(np.arange(10, 30), log["user_idx"][got]).any()          # the users of 1 and of 2 rows go


@pytest.mark.parametrize("ts_kind", KINDS)
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("days", [0, 1, 3, 10 ** 6])
def test_day_filters_grid(days, first, ts_kind):
    log = half_days(ts_kind)
    dev = given(log, ts_kind, "half_" + ts_kind)
    n = len(log["user_idx"])
    by_user = check("take_num_days_of_user_hist", dict(days=days, first=first), log, dev)
    whole = check("take_num_days_of_global_hist", dict(duration_days=days, first=first), log, dev)
    assert (len(by_user), len(whole)) == {0: (0, 0), 10 ** 6: (n, n)}.get(days, (len(by_user), len(whole)))
    if days in (1, 3):
        # rows exactly on the bound exist and are out (first: ts < min + days; last: ts > max - days)
        ts = log["timestamp"]
        sec = ts.astype("datetime64[ns]").astype(np.int64) // 10 ** 9 if ts_kind == "datetime" else ts
        bound = sec.min() + 86400 * days if first else sec.max() - 86400 * days
        on_bound = np.flatnonzero(sec == bound)
        assert len(on_bound) > 0 and not np.isin(on_bound, whole).any()
        assert 0 < len(whole) < n and len(whole) <= len(by_user) < n


PERIODS = {
    "int": [(None, None), ("2019-09-20", None), (None, "2019-09-20"), ("2019-09-10", "2019-09-20 00:00:00"),
            (datetime(2019, 9, 20), datetime(2019, 9, 20, 0, 0, 0, 5)), (datetime(2019, 9, 20, 0, 0, 0, 5), None),
            (SR.DAY0 + 19 * 86400, SR.DAY0 + 19 * 86400), ("2019-09-21", "2019-09-20"), (SR.DAY0 - 1, SR.DAY0 + 500 * 86400),
            (None, SR.DAY0), (SR.DAY0 + 49 * 86400, None)],
    "float": [(None, None), (0, None), (None, 0), (-3, 5), (0, 0), (5, -3), (-100, 100)],
    "datetime": [(None, None), ("2019-09-20", None), (None, "2019-09-20"), ("2019-09-10 00:00:00", datetime(2019, 9, 20)),
                 (datetime(2019, 9, 20), datetime(2019, 9, 20, 0, 0, 0, 5)), (datetime(2019, 9, 20, 0, 0, 0, 5), None),
                 (SR.DAY0 + 19 * 86400, SR.DAY0 + 19 * 86400), ("2019-09-21", "2019-09-20")],
}


@pytest.mark.parametrize("ts_kind", KINDS)
def test_take_time_period_bounds(ts_kind):
    log = edge(ts_kind)
    dev = given(log, ts_kind, ts_kind)
    n = len(log["user_idx"])
    sizes = [len(check("take_time_period", dict(start_date=a, end_date=b), log, dev)) for a, b in PERIODS[ts_kind]]
    assert sizes[0] == n and sizes[1] + sizes[2] == n and 0 < sizes[1] < n          # a bound ON a timestamp cuts once
    assert 0 < sizes[3] < n
    if ts_kind == "float":
        assert (log["timestamp"] == 0.0).any() and sizes[4] == 0 and sizes[5] == 0 and sizes[6] == n
    else:
        day = np.datetime64("2019-09-20") if ts_kind == "datetime" else SR.DAY0 + 19 * 86400
        assert sizes[4] == (log["timestamp"] == day).sum() > 0                       # 5 us wide: that timestamp alone
        assert sizes[5] == sizes[1] - sizes[4]                                       # the least key NOT BEFORE the bound
        assert sizes[6] == 0 and sizes[7] == 0                                       # empty periods


@pytest.mark.parametrize("value", [0.0, -0.0, 0.5, 0.75, 2.0, 2.5, -1.0, float("nan"), float("inf"), float("-inf")])
def test_filter_out_low_ratings(value):
    log = edge()
    rel = log["relevance"]
    assert np.isnan(rel).any() and (np.signbit(rel) & (rel == 0)).any() and (~np.signbit(rel) & (rel == 0)).any()
    got = check("filter_out_low_ratings", dict(value=value), log, on_device(log, "int"))
    assert not np.isnan(rel[got]).any()                                              # a NaN row is dropped, always
    if value == 0.0:
        assert (rel == 0).sum() == (rel[got] == 0).sum() > 0                         # the threshold itself and -0.0 stay
    # another column, another dtype: an integer rating
    other = dict(log, stars=(np.nan_to_num(rel) * 2).astype(np.int32))
    got = F.filter_out_low_ratings(on_device(other), 2, rating_column="stars", return_rows=True).cpu().numpy()
    assert np.array_equal(got, np.flatnonzero(other["stars"] >= 2))


# ---------------------------------------------------------------------------------------------------------------------
# small logs
# ---------------------------------------------------------------------------------------------------------------------
ALL = [("filter_by_min_count", dict(num_entries=1)), ("filter_out_low_ratings", dict(value=0.5)),
       ("take_num_user_interactions", dict(num_interactions=1)), ("take_num_user_interactions", dict(first=False, item_col=None)),
       ("take_num_days_of_user_hist", dict(days=1)), ("take_num_days_of_user_hist", dict(days=1, first=False)),
       ("take_time_period", dict(start_date=17, end_date=18)), ("take_time_period", {}),
       ("take_num_days_of_global_hist", dict(duration_days=1)), ("take_num_days_of_global_hist", dict(duration_days=1, first=False))]


def test_empty_and_single_row_logs(caplog):
    cols = {"user_idx": np.zeros(0, np.int64), "item_idx": np.zeros(0, np.int64), "timestamp": np.zeros(0, np.int64),
            "relevance": np.zeros(0, np.float64)}
    one = {"user_idx": np.array([4]), "item_idx": np.array([2]), "timestamp": np.array([17]), "relevance": np.array([1.0])}
    with caplog.at_level(logging.INFO, logger="replay"):
        for name, args in ALL:
            out = getattr(F, name)(pd.DataFrame(cols), **args)
            assert isinstance(out, pd.DataFrame) and len(out) == 0 and list(out.columns) == list(cols)
            rows = getattr(F, name)(on_device(cols), **args, return_rows=True)
            assert rows.numel() == 0 and rows.dtype == torch.int64 and rows.is_cuda
    assert not caplog.records                                                        # an empty log logs nothing
    for name, args in ALL:
        assert check(name, args, one, on_device(one)).tolist() == [0]
    assert check("filter_by_min_count", dict(num_entries=2), one, on_device(one)).tolist() == []
    assert check("take_num_days_of_global_hist", dict(duration_days=0), one, on_device(one)).tolist() == []
    # ids are range-checked before any kernel indexes with them
    with pytest.raises(ValueError, match="non-negative"):
        F.filter_by_min_count(on_device(dict(one, user_idx=np.array([-1]))), 1)
    with pytest.raises(ValueError, match="non-negative"):
        F.take_num_user_interactions(on_device(dict(one, item_idx=np.array([-5]))), 1)
    with pytest.raises(ValueError, match="below 2"):
        F.take_num_days_of_user_hist(on_device(dict(one, user_idx=np.array([2 ** 31 - 1]))), 1)
    with pytest.raises(ValueError, match="NaN"):
        F.take_num_days_of_global_hist(on_device(dict(one, timestamp=np.array([np.nan]))), 1)


def test_one_user_holds_all_rows():
    rng = np.random.default_rng(3)
    n = 2049
    log = {"user_idx": np.full(n, 5, np.int64), "item_idx": rng.integers(0, 3, n), "timestamp": rng.integers(0, 4, n) * 43200,
           "relevance": rng.random(n)}
    dev = on_device(log)
    for first in (True, False):
        for k in (1, 1000, n, n + 1):
            for item_col in ("item_idx", None):
                check("take_num_user_interactions", dict(num_interactions=k, first=first, item_col=item_col), log, dev)
        check("take_num_days_of_user_hist", dict(days=1, first=first), log, dev)
    assert len(check("filter_by_min_count", dict(num_entries=n), log, dev)) == n
    assert len(check("filter_by_min_count", dict(num_entries=n + 1), log, dev)) == 0


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("days", [1, 10 ** 5, 10 ** 13, 10 ** 18, 10 ** 30, -1, -10 ** 30])
def test_int64_timestamps_near_the_limits_saturate(days, first):
    top, low = (1 << 63) - 1, -(1 << 63)
    ts = np.array([top - 5, top, low, low + 5, top - 86400, low + 86400, 0, top - 86401, low + 86401], dtype=np.int64)
    log = {"user_idx": np.array([0, 0, 1, 1, 0, 1, 2, 0, 1]), "timestamp": ts}
    dev = on_device(log)
    check("take_num_days_of_user_hist", dict(days=days, first=first), log, dev)
    check("take_num_days_of_global_hist", dict(duration_days=days, first=first), log, dev)
    # a datetime column is compared in ns: the span is 10^9 larger, and 10^5 days past +-4.6e18 ns leave int64 already
    far = {"user_idx": log["user_idx"], "timestamp": (ts // (2 * 10 ** 9)).astype("datetime64[s]").astype("datetime64[ns]")}
    check("take_num_days_of_user_hist", dict(days=days, first=first), far, pd.DataFrame(far))
    check("take_num_days_of_global_hist", dict(duration_days=days, first=first), far, pd.DataFrame(far))


def _frame():
    log = SR.edge_log(n_rows=5001, n_users=400, big=600, n_days=11, ts_kind="datetime")
    frame = pd.DataFrame({"user_idx": log["user_idx"].astype(np.int32), "item_idx": log["item_idx"].astype(np.int16),
                          "timestamp": log["timestamp"], "relevance": log["relevance"].astype(np.float32)})
    frame["note"] = [f"row{i}" for i in range(len(frame))]               # an extra column, not even numeric
    frame["weight"] = np.arange(len(frame), dtype=np.float64) * 0.5
    frame.index = frame.index[::-1]                                      # an index the output must not carry
    return log, frame


@pytest.mark.parametrize("name,args", [("take_num_user_interactions", dict(num_interactions=3, first=False)),
                                       ("filter_by_min_count", dict(num_entries=12)),
                                       ("take_time_period", dict(start_date="2019-09-03", end_date="2019-09-08"))])
def test_the_kind_that_goes_in_comes_out_with_every_column(name, args):
    log, frame = _frame()
    want = R.keep_rows(name, args, log)
    assert 0 < len(want) < len(frame)
    fn = getattr(F, name)
    got = fn(frame, **args)
    assert isinstance(got, pd.DataFrame) and dict(got.dtypes) == dict(frame.dtypes)
    pd.testing.assert_frame_equal(got, frame.iloc[want].reset_index(drop=True))          # values, dtypes, fresh index
    table = pa.Table.from_pandas(frame, preserve_index=False)
    for src, kind in ((table, pa.Table), (table.combine_chunks().to_batches()[0], pa.RecordBatch),
                      (table.to_batches(max_chunksize=700), pa.Table), (iter(table.to_batches(max_chunksize=700)), pa.Table)):
        got = fn(src, **args)
        assert isinstance(got, kind) and got.schema.equals(table.schema)
        assert got.to_pydict() == table.take(pa.array(want)).to_pydict()
    # device tensors, custom column names, one extra column and one entry that is no tensor
    dev = {"u": torch.as_tensor(log["user_idx"]).to(DEV), "i": torch.as_tensor(log["item_idx"].astype(np.int32)).to(DEV),
           "t": torch.as_tensor(log["timestamp"].astype("datetime64[s]").astype(np.int64)).to(DEV),
           "extra": torch.arange(len(frame), dtype=torch.float16, device=DEV), "name": "my log"}
    renamed = {"take_num_user_interactions": dict(user_col="u", item_col="i", date_col="t"),
               "filter_by_min_count": dict(group_by="u"), "take_time_period": dict(date_column="t")}[name]
    got = fn(dev, **args, **renamed)
    assert set(got) == set(dev) and got["name"] == "my log"
    for k, v in dev.items():
        if torch.is_tensor(v):
            assert got[k].is_cuda and got[k].dtype == v.dtype and torch.equal(got[k].cpu(), v.cpu()[torch.as_tensor(want)])
    rows = fn(dev, **args, **renamed, return_rows=True)
    assert rows.dtype == torch.int64 and rows.is_cuda and np.array_equal(rows.cpu().numpy(), want)
    with pytest.raises(ValueError, match="no column"):
        fn(dev, **args)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_known_answers_through_the_device_path(case):
    log = R.golden_log(case["log"])
    frame = pd.DataFrame(log)
    got = getattr(F, case["filter"])(frame, **R.golden_args(case["args"]))
    assert isinstance(got, pd.DataFrame) and list(got.columns) == list(log)
    pd.testing.assert_frame_equal(got, frame.iloc[case["kept_rows"]].reset_index(drop=True))
    rows = getattr(F, case["filter"])(frame, **R.golden_args(case["args"]), return_rows=True)
    assert rows.cpu().tolist() == case["kept_rows"]


def test_known_answer_of_the_indexer():
    g = GOLDEN["indexer"]
    frame = pd.DataFrame(g["frame"])
    ix = Indexer(g["user_col"], g["item_col"])
    ix.fit(frame, frame)
    res = ix.transform(frame)
    assert list(res.columns) == ["user_idx", "item_idx"] and res.to_dict("list") == g["transformed"]
    assert res.user_idx.dtype == np.int32 and res.item_idx.dtype == np.int32
    pd.testing.assert_frame_equal(ix.inverse_transform(res), frame)


def test_removed_share_is_logged_at_both_levels(caplog):
    log = edge()
    dev = on_device(log, "int")
    n = len(log["user_idx"])
    for num_entries, level in ((2, "INFO"), (5000, "WARNING")):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="replay"):
            kept = F.filter_by_min_count(dev, num_entries, return_rows=True).numel()
        records = [r for r in caplog.records if r.name == "replay"]
        assert len(records) == 1 and records[0].levelname == level
        share = (n - kept) / n
        assert (share > 0.5) == (level == "WARNING")
        assert records[0].getMessage() == f"current threshold removes {share}% of data"


def test_two_calls_return_identical_bytes():
    log = half_days("float")
    dev = on_device(log, "half_float")
    for name, args in (("take_num_user_interactions", dict(num_interactions=7, first=False)),
                       ("take_num_user_interactions", dict(num_interactions=7, item_col=None)),
                       ("filter_by_min_count", dict(num_entries=20, group_by="item_idx")),
                       ("take_num_days_of_user_hist", dict(days=3, first=False)),
                       ("take_num_days_of_global_hist", dict(duration_days=3)),
                       ("filter_out_low_ratings", dict(value=0.5)), ("take_time_period", dict(start_date=-2000000, end_date=-1000000))):
        first = getattr(F, name)(dev, **args, return_rows=True).cpu().numpy().tobytes()
        again = getattr(F, name)(dev, **args, return_rows=True).cpu().numpy().tobytes()
        assert first == again and len(first) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the Indexer
# ---------------------------------------------------------------------------------------------------------------------
def raw_log():
    """70 001 rows of sparse int64 ids, negative ones among them: data._mix64 of a counter"""
    if "raw" not in _LOGS:
        rng = np.random.default_rng(11)
        users = D._mix64(torch.arange(3000, dtype=torch.int64)).numpy()
        items = D._mix64(torch.arange(10 ** 6, 10 ** 6 + 1000, dtype=torch.int64)).numpy()
        assert (users < 0).any() and (users > 2 ** 40).any() and len(np.unique(users)) == 3000
        n = 70001
        _LOGS["raw"] = {"user_id": users[rng.integers(0, 3000, n)], "item_id": items[rng.integers(0, 1000, n)],
                        "relevance": rng.random(n), "timestamp": rng.integers(0, 50, n)}
    return _LOGS["raw"]


def test_indexer_fit_transform_inverse_on_sparse_and_negative_ids():
    log = raw_log()
    dev = on_device(log, "raw")
    ref = R.DictIndexer()
    ref.fit(log["user_id"], log["item_id"])
    ix = Indexer()
    ix.fit(dev, dev)
    assert ix.user_labels.dtype == torch.int64 and ix.user_labels.is_cuda
    assert ix.user_labels.cpu().tolist() == ref.labels["user"] and ix.item_labels.cpu().tolist() == ref.labels["item"]
    res = ix.transform(dev)
    assert list(res) == ["user_idx", "item_idx", "relevance", "timestamp"]
    assert res["user_idx"].dtype == torch.int32 and res["item_idx"].dtype == torch.int32 and res["user_idx"].is_cuda
    u, i = res["user_idx"].cpu().numpy(), res["item_idx"].cpu().numpy()
    assert np.array_equal(u, ref.transform("user", log["user_id"])) and np.array_equal(i, ref.transform("item", log["item_id"]))
    m_u, m_i = len(np.unique(log["user_id"])), len(np.unique(log["item_id"]))
    assert np.array_equal(np.unique(u), np.arange(m_u)) and np.array_equal(np.unique(i), np.arange(m_i))  # exactly 0..m-1
    assert torch.equal(res["relevance"], dev["relevance"])
    back = ix.inverse_transform(res)
    assert list(back) == ["user_id", "item_id", "relevance", "timestamp"]
    for col in ("user_id", "item_id"):
        assert back[col].dtype == torch.int64 and torch.equal(back[col], dev[col])
    # twice the same bytes
    again = ix.transform(dev)
    assert torch.equal(again["user_idx"], res["user_idx"]) and torch.equal(again["item_idx"], res["item_idx"])


def test_indexer_round_trip_keeps_the_kind_and_the_dtype():
    log = raw_log()
    frame = pd.DataFrame({"user_id": (log["user_id"][:5001] >> 33).astype(np.int32), "item_id": log["item_id"][:5001],
                          "note": [f"row{k}" for k in range(5001)], "relevance": log["relevance"][:5001]})
    frame.index = frame.index[::-1]
    assert (frame.user_id < 0).any()
    ix = Indexer()
    ix.fit(frame[["user_id"]], frame[["item_id"]])
    assert ix.user_type == np.int32 and ix.item_type == np.int64
    ref = R.DictIndexer()
    ref.fit(frame.user_id, frame.item_id)
    res = ix.transform(frame)
    assert isinstance(res, pd.DataFrame) and list(res.columns) == ["user_idx", "item_idx", "note", "relevance"]
    assert res.user_idx.dtype == np.int32 and res.item_idx.dtype == np.int32 and list(res.index) == list(range(5001))
    assert np.array_equal(res.user_idx, ref.transform("user", frame.user_id)) and list(res.note) == list(frame.note)
    back = ix.inverse_transform(res)
    pd.testing.assert_frame_equal(back, frame.reset_index(drop=True))                   # values AND dtypes (int32 / int64)
    table = pa.Table.from_pandas(frame, preserve_index=False)
    for src, kind in ((table, pa.Table), (table.combine_chunks().to_batches()[0], pa.RecordBatch),
                      (table.to_batches(max_chunksize=700), pa.Table)):
        res_a = ix.transform(src)
        assert isinstance(res_a, kind) and res_a.schema.names == ["user_idx", "item_idx", "note", "relevance"]
        assert res_a.schema.field("user_idx").type == pa.int32() and res_a.column(0).to_pylist() == res.user_idx.tolist()
        back_a = ix.inverse_transform(res_a)
        assert isinstance(back_a, kind) and back_a.schema.equals(table.schema) and back_a.to_pydict() == table.to_pydict()
    # a dict of device tensors with int32 raw ids comes back as int32 tensors
    dev = {"user_id": torch.as_tensor(frame.user_id.to_numpy()).to(DEV), "item_id": torch.as_tensor(frame.item_id.to_numpy()).to(DEV)}
    back_d = ix.inverse_transform(ix.transform(dev))
    assert back_d["user_id"].dtype == torch.int32 and torch.equal(back_d["user_id"], dev["user_id"])
    assert back_d["item_id"].dtype == torch.int64 and torch.equal(back_d["item_id"], dev["item_id"])


def test_indexer_appends_unseen_ids_ascending_and_moves_no_index():
    log = raw_log()
    dev = on_device(log, "raw")
    seen = {k: v[log["user_id"] % 3 != 0] for k, v in log.items()}                      # a third of the users unseen
    seen = {k: v[seen["item_id"] % 5 != 0] for k, v in seen.items()}
    ref = R.DictIndexer()
    ref.fit(seen["user_id"], seen["item_id"])
    ix = Indexer()
    ix.fit(on_device(seen), on_device(seen))
    old_users, old_items = ix.user_labels.clone(), ix.item_labels.clone()
    assert old_users.numel() < 3000
    before = ix.transform(on_device(seen))
    res = ix.transform(dev)
    assert np.array_equal(res["user_idx"].cpu().numpy(), ref.transform("user", log["user_id"]))
    assert np.array_equal(res["item_idx"].cpu().numpy(), ref.transform("item", log["item_id"]))
    assert ix.user_labels.cpu().tolist() == ref.labels["user"] and ix.item_labels.cpu().tolist() == ref.labels["item"]
    assert torch.equal(ix.user_labels[:old_users.numel()], old_users) and torch.equal(ix.item_labels[:old_items.numel()], old_items)
    new = ix.user_labels[old_users.numel():].cpu().numpy()
    assert len(new) == 3000 - old_users.numel() and (np.diff(new) > 0).all()           # appended in ascending id order
    after = ix.transform(on_device(seen))
    assert torch.equal(after["user_idx"], before["user_idx"]) and torch.equal(after["item_idx"], before["item_idx"])
    back = ix.inverse_transform(res)
    assert torch.equal(back["user_id"], dev["user_id"]) and torch.equal(back["item_id"], dev["item_id"])


def test_indexer_with_one_of_the_two_columns_and_bad_indices():
    log = raw_log()
    dev = on_device(log, "raw")
    ix = Indexer()
    ix.fit(dev, dev)
    only_items = ix.transform({"item_id": dev["item_id"], "relevance": dev["relevance"]})
    assert list(only_items) == ["item_idx", "relevance"] and only_items["item_idx"].dtype == torch.int32
    only_users = ix.transform(pd.DataFrame({"w": [1.5, 2.5], "user_id": log["user_id"][:2]}))
    assert list(only_users.columns) == ["user_idx", "w"]
    assert list(ix.inverse_transform(only_items)) == ["item_id", "relevance"]
    assert list(ix.inverse_transform(only_users).columns) == ["user_id", "w"]
    neither = ix.transform(pd.DataFrame({"w": [1.5, 2.5]}))
    assert list(neither.columns) == ["w"] and len(neither) == 2
    m = ix.item_labels.numel()
    for bad in (m, -1, 2 ** 40):
        with pytest.raises(ValueError, match="outside"):
            ix.inverse_transform({"item_idx": torch.tensor([0, bad, 1], device=DEV)})
    assert ix.inverse_transform({"item_idx": torch.tensor([m - 1], device=DEV)})["item_id"].item() == ix.item_labels[-1].item()
    empty = ix.transform({"user_id": torch.empty(0, dtype=torch.int64, device=DEV)})
    assert empty["user_idx"].numel() == 0 and empty["user_idx"].dtype == torch.int32
    fresh = Indexer()
    fresh.fit({"user_id": torch.empty(0, dtype=torch.int64, device=DEV)}, {"item_id": torch.empty(0, dtype=torch.int64, device=DEV)})
    assert fresh.user_labels.numel() == 0
    assert fresh.transform({"user_id": torch.tensor([9, -9, 9], device=DEV)})["user_idx"].cpu().tolist() == [1, 0, 1]


# ---------------------------------------------------------------------------------------------------------------------
# filters -> Indexer -> splitter
# ---------------------------------------------------------------------------------------------------------------------
def test_pipeline_filters_indexer_splitter():
    raw = raw_log()
    rng = np.random.default_rng(5)
    log = dict(raw, relevance=rng.choice(np.array([0.0, 0.5, 1.0, 2.0, np.nan]), len(raw["user_id"])))
    # the filters want dense group ids: the raw log goes through an Indexer first, as a RePlay experiment does
    first_ix, ref_first = Indexer(), R.DictIndexer()
    first_ix.fit(on_device(log), on_device(log))
    ref_first.fit(log["user_id"], log["item_id"])
    dense = first_ix.transform(on_device(log))
    want = {"user_idx": ref_first.transform("user", log["user_id"]).astype(np.int64),
            "item_idx": ref_first.transform("item", log["item_id"]).astype(np.int64),
            "relevance": log["relevance"], "timestamp": log["timestamp"]}
    # device: low ratings out, 20-core on users, re-index (the filter left holes), last row of every user is test
    step1 = F.filter_out_low_ratings(dense, 0.5)
    step2 = F.filter_by_min_count(step1, 20)
    ix = Indexer("user_idx", "item_idx")
    ix.fit(step2, step2)
    step3 = ix.transform(step2)
    train, test = S.UserSplitter(item_test_size=1).split(step3)
    # numpy: the references composed
    rows1 = R.keep_rows("filter_out_low_ratings", dict(value=0.5), want)
    want1 = {k: v[rows1] for k, v in want.items()}
    rows2 = R.keep_rows("filter_by_min_count", dict(num_entries=20), want1)
    want2 = {k: v[rows2] for k, v in want1.items()}
    assert 0 < len(rows2) < len(rows1) < len(log["user_id"])
    ref = R.DictIndexer()
    ref.fit(want2["user_idx"], want2["item_idx"])
    want3 = dict(want2, user_idx=ref.transform("user", want2["user_idx"]).astype(np.int64),
                 item_idx=ref.transform("item", want2["item_idx"]).astype(np.int64))
    assert want3["user_idx"].max() + 1 == len(np.unique(want2["user_idx"])) < want2["user_idx"].max() + 1    # holes closed
    train_rows, test_rows = SR.split_rows("UserSplitter", dict(item_test_size=1), want3)
    assert len(test_rows) > 0
    for got, rows in ((train, train_rows), (test, test_rows)):
        assert list(got) == ["user_idx", "item_idx", "relevance", "timestamp"]
        for col in got:
            assert np.array_equal(got[col].cpu().numpy(), want3[col][rows]), col
