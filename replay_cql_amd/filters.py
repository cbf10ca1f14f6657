"""The filters of replay/filters.py on the GPU: filter_by_min_count, filter_out_low_ratings, take_num_user_interactions,
take_num_days_of_user_hist, take_time_period and take_num_days_of_global_hist, with the reference's names, argument
names, order and defaults.  What the reference does with Spark window passes and joins is a count or an extreme per
group, a ranking inside each user, one row predicate and a stable compaction here -- csrc/prepare.hip, integer work
throughout, deterministic.

Every filter takes what the splitters take -- a pandas DataFrame, a pyarrow Table / RecordBatch / sequence of batches,
or a dict of device tensors -- and returns the kind it was given (a sequence of batches comes back as a Table): every
column carried, rows in input order, the pandas index reset.  The keyword-only `return_rows=True` returns the ascending
int64 device tensor of the kept input row indices instead.  An empty log comes back empty without a launch; a log of
2^31 rows or more raises ValueError.  Importing this module needs no GPU; calling a filter without one raises
CqlrecError.  Filtering leaves holes in the id space: put indexer.Indexer behind it.

Semantics, and where they deviate from the reference on purpose:
  * filter_by_min_count keeps a row iff its `group_by` value occurs >= num_entries times.  The group column is an
    integer column of non-negative ids below 2^31 - 1 (range-checked before any launch; the counts are an array indexed
    by the id).  The removed share is logged as the reference logs it ("current threshold removes ...": warning above
    0.5, info otherwise, on the "replay" logger); an empty log logs nothing.
  * filter_out_low_ratings keeps a row iff float64(column) >= value under IEEE comparison, so a NaN row is DROPPED
    (Spark orders NaN above every number and would keep it).
  * take_num_user_interactions orders the rows of each user by (timestamp key, item, input row index) ascending -- the
    item is left out when item_col is None.  first=True keeps the first num_interactions rows of that order; first=False
    keeps the first num_interactions rows of its EXACT REVERSE, so among fully equal rows the later input row is the
    more recent one (the splitters' rule; the reference leaves such ties to Spark).  Hence, for a user of c rows,
    (first=True, n) and (first=False, c - n) partition the user's rows.  num_interactions <= 0 keeps nothing.  user_col
    and item_col are integer columns of non-negative ids below 2^31 - 1.
  * days.  One day is 86 400 s (Spark's INTERVAL n days follows the session time zone's calendar).  `days` /
    `duration_days` must be integral (numbers.Integral, not bool), else ValueError.  datetime and integer timestamp
    columns: the span days * 86400 (* 10^9 for datetime columns, which are compared in ns) and the bound extreme +/- span
    are computed in int64, each saturating at the int64 limits.  float columns: the extreme is found on the
    order-preserving key (data.timestamp_key) and decoded back to the double; the bound is ONE IEEE double add or
    subtract of 86400.0 * days, and the comparison is made in double.
  * take_num_days_of_user_hist: first keeps ts < min_u + days, otherwise ts > max_u - days (min_u / max_u over the
    user's rows); take_num_days_of_global_hist: the same with the log's global min / max.
  * take_time_period keeps start <= ts < end; None is unbounded on that side (the reference's defaults, min and
    max + 1 s, keep every row: the same thing).  A bound is a datetime (naive = UTC), a "yyyy-MM-dd[ HH:mm:ss]" string
    or an int of unix seconds, turned by splitters._threshold_key into the least key of the column's dtype whose value
    is >= the bound."""
from __future__ import annotations

import logging
import math
import numbers
from datetime import datetime
from typing import Optional, Union

import torch

from . import _log as L
from . import _native as N
from . import _prepare as P
from .splitters import _instant_ns, _threshold_key

__all__ = ["filter_by_min_count", "filter_out_low_ratings", "take_num_user_interactions", "take_num_days_of_user_hist",
           "take_time_period", "take_num_days_of_global_hist"]

DAY_S = 86400


def _logger():
    return logging.getLogger("replay")          # the reference's State().logger


def _need(log, name, kinds: str, what: str) -> None:
    kind, _ = L.column_kind(log, name)
    if kind not in kinds:
        raise ValueError(f"column {name} must be {what}")


def _id_column(log, name) -> None:
    _need(log, name, "iu", "an integer column")


def _date_column(log, name) -> None:
    _need(log, name, "Miuf", "a datetime, integer or float column")


def _integral_days(days, name: str) -> int:
    if not isinstance(days, numbers.Integral) or isinstance(days, bool):
        raise ValueError(f"{name} must be an integer number of days, got {days!r}")
    return int(days)


def _no_rows(lg):
    return torch.empty(0, dtype=torch.int64, device=lg.device)


def _result(lg, rows, return_rows: bool):
    return rows if return_rows else lg.take(rows)


def _spans(days: int, ts_kind: str):
    """(int64 span in the column's unit, saturated; double span in seconds)"""
    try:
        x = 86400.0 * float(days)
    except OverflowError:
        x = math.copysign(math.inf, days)
    return L.clip64(days * DAY_S * (10 ** 9 if ts_kind == "datetime" else 1)), x


def filter_by_min_count(data_frame, num_entries: int, group_by: str = "user_idx", *, return_rows: bool = False):
    """Remove the rows whose `group_by` value occurs fewer than `num_entries` times in `data_frame`."""
    src = L.normalise(data_frame)
    _id_column(src, group_by)
    lg = L.open_log(src, "filter_by_min_count")
    if lg.n == 0:
        return _result(lg, _no_rows(lg), return_rows)
    (group, n_groups), = L.dense_ids(lg, [group_by])
    prep = P.Prep(lg.device)
    count = prep.count(group, n_groups)
    rows = prep.compact(prep.keep(N.KEEP_MIN_COUNT, lg.n, group=group, count=count,
                                  n=L.clip64(math.ceil(num_entries))))
    diff = (lg.n - rows.numel()) / lg.n
    (_logger().warning if diff > 0.5 else _logger().info)("current threshold removes %s%% of data", diff)
    return _result(lg, rows, return_rows)


def filter_out_low_ratings(data_frame, value: float, rating_column="relevance", *, return_rows: bool = False):
    """Remove the rows whose `rating_column` is less than `value` (or NaN)."""
    src = L.normalise(data_frame)
    _need(src, rating_column, "iufb", "a numeric column")
    value = float(value)
    lg = L.open_log(src, "filter_out_low_ratings")
    if lg.n == 0:
        return _result(lg, _no_rows(lg), return_rows)
    prep = P.Prep(lg.device)
    rows = prep.compact(prep.keep(N.KEEP_MIN_VALUE, lg.n, value=L.float_column(lg, rating_column), x=value))
    return _result(lg, rows, return_rows)


# pylint: disable=too-many-arguments
def take_num_user_interactions(log, num_interactions: int = 10, first: bool = True, date_col: str = "timestamp",
                               user_col: str = "user_idx", item_col: Optional[str] = "item_idx", *,
                               return_rows: bool = False):
    """The first / last `num_interactions` rows of each user by (date_col, item_col, input row)."""
    src = L.normalise(log)
    _id_column(src, user_col)
    if item_col is not None:
        _id_column(src, item_col)
    _date_column(src, date_col)
    n = L.clip64(math.floor(num_interactions))
    lg = L.open_log(src, "take_num_user_interactions")
    if lg.n == 0 or n <= 0:
        return _result(lg, _no_rows(lg), return_rows)
    ids = L.dense_ids(lg, [user_col] + ([item_col] if item_col is not None else []))
    (user, n_users), (item, n_items) = ids[0], (ids[1] if item_col is not None else (None, 0))
    prep = P.Prep(lg.device)
    rank, count = prep.rank(user, n_users, lg.key(date_col), item, n_items)
    rows = prep.compact(prep.keep(N.KEEP_NUM_INTERACTIONS, lg.n, group=user, rank=rank, count=count, n=n, first=bool(first)))
    return _result(lg, rows, return_rows)


def _days(lg, prep, rule, key, group, n_groups, days: int, first: bool):
    lo, hi = prep.minmax(group, n_groups, key)
    span, x = _spans(days, lg.ts_kind)
    return prep.compact(prep.keep(rule, lg.n, group=group, key=key, extreme=lo if first else hi, n=span, first=first,
                                  float_key=lg.ts_kind == "float", x=x))


def take_num_days_of_user_hist(log, days: int = 10, first: bool = True, date_col: str = "timestamp",
                               user_col: str = "user_idx", *, return_rows: bool = False):
    """The first / last `days` days of each user's history, counted from the user's own first / last timestamp."""
    days = _integral_days(days, "days")
    src = L.normalise(log)
    _id_column(src, user_col)
    _date_column(src, date_col)
    lg = L.open_log(src, "take_num_days_of_user_hist")
    if lg.n == 0:
        return _result(lg, _no_rows(lg), return_rows)
    (user, n_users), = L.dense_ids(lg, [user_col])
    rows = _days(lg, P.Prep(lg.device), N.KEEP_DAYS_USER, lg.key(date_col), user, n_users, days, bool(first))
    return _result(lg, rows, return_rows)


def take_time_period(log, start_date: Optional[Union[str, datetime]] = None,
                     end_date: Optional[Union[str, datetime]] = None, date_column: str = "timestamp", *,
                     return_rows: bool = False):
    """The rows with start_date <= date_column < end_date."""
    for bound in (start_date, end_date):
        if bound is not None:
            _instant_ns(bound)                   # ValueError for a form or a string that is no date
    src = L.normalise(log)
    _date_column(src, date_column)
    lg = L.open_log(src, "take_time_period")
    if lg.n == 0:
        return _result(lg, _no_rows(lg), return_rows)
    key = lg.key(date_column)
    lo = L.I64_MIN if start_date is None else L.clip64(_threshold_key(start_date, lg.ts_kind))
    hi = 0 if end_date is None else L.clip64(_threshold_key(end_date, lg.ts_kind))
    prep = P.Prep(lg.device)
    rows = prep.compact(prep.keep(N.KEEP_PERIOD, lg.n, key=key, lo=lo, hi=hi, open_end=end_date is None))
    return _result(lg, rows, return_rows)


def take_num_days_of_global_hist(log, duration_days: int, first: bool = True, date_column: str = "timestamp", *,
                                 return_rows: bool = False):
    """The first / last `duration_days` days of the log, counted from its first / last timestamp."""
    days = _integral_days(duration_days, "duration_days")
    src = L.normalise(log)
    _date_column(src, date_column)
    lg = L.open_log(src, "take_num_days_of_global_hist")
    if lg.n == 0:
        return _result(lg, _no_rows(lg), return_rows)
    rows = _days(lg, P.Prep(lg.device), N.KEEP_DAYS_GLOBAL, lg.key(date_column), None, 1, days, bool(first))
    return _result(lg, rows, return_rows)
