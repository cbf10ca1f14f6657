"""Plain numpy implementation of the filter semantics of replay_cql_amd/filters.py and a dict-based Indexer, written from
their definition (not from the device code): the yardstick of tests/test_gpu_filters.py, checked itself against the
known answers of tests/golden/filters_known_answers.json and brute force by tests/test_filter_reference_cpu.py.

A log is a dict of numpy columns (user_idx, item_idx, relevance, timestamp: int64, float64 or datetime64, and any others).
`keep_rows(name, args, log)` -> ascending int64 input row indices of the rows the filter keeps."""
from __future__ import annotations

import math
import numbers
from datetime import datetime
from fractions import Fraction

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DAY_S = 86400


def _sat(x: int) -> int:
    return max(I64_MIN, min(I64_MAX, int(x)))


def _seconds(bound) -> Fraction:
    """a datetime (naive = UTC), "yyyy-MM-dd[ HH:mm:ss]" or int unix seconds as an exact number of seconds"""
    if isinstance(bound, str):
        return Fraction(int(np.datetime64(bound).astype("datetime64[s]").astype(np.int64)))
    if isinstance(bound, datetime):
        whole = np.datetime64(bound.replace(microsecond=0, tzinfo=None)).astype("datetime64[s]").astype(np.int64)
        return Fraction(int(whole)) + Fraction(bound.microsecond, 10 ** 6)
    if isinstance(bound, numbers.Integral) and not isinstance(bound, bool):
        return Fraction(int(bound))
    raise ValueError(f"not a date: {bound!r}")


def _at_or_after(ts, bound):
    """ts >= bound, exactly, for each dtype of a timestamp column"""
    sec = _seconds(bound)
    if ts.dtype.kind == "M":
        ns = ts.astype("datetime64[ns]").astype(np.int64)
        return ns >= _sat(math.ceil(sec * 10 ** 9))
    if ts.dtype.kind in "iu":
        return ts.astype(np.int64) >= _sat(math.ceil(sec))
    return ts.astype(np.float64) >= float(sec)


def _order_in_user(user, ts, item):
    """rows sorted by (user, timestamp, item, input row) ascending + position of every row inside its user + rows per user"""
    n = len(user)
    keys = (np.arange(n),) + ((item,) if item is not None else ()) + (ts, user)
    order = np.lexsort(keys)
    counts = np.bincount(user, minlength=int(user.max()) + 1 if n else 0).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(counts) else counts
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    return pos - starts[user], counts[user]


def _days_mask(ts, extreme, days, first):
    """ts < extreme + days (first) or ts > extreme - days, one day = 86 400 s; `extreme` per row or a scalar"""
    if not isinstance(days, numbers.Integral) or isinstance(days, bool):
        raise ValueError("days must be integral")
    days = int(days)
    if ts.dtype.kind == "f":
        span = np.float64(86400.0) * np.float64(days)
        with np.errstate(over="ignore", invalid="ignore"):
            return ts < extreme + span if first else ts > extreme - span
    unit = 10 ** 9 if ts.dtype.kind == "M" else 1
    t = ts.astype("datetime64[ns]").astype(np.int64) if ts.dtype.kind == "M" else ts.astype(np.int64)
    e = np.broadcast_to(np.asarray(extreme).astype("datetime64[ns]").astype(np.int64) if ts.dtype.kind == "M"
                        else np.asarray(extreme, dtype=np.int64), t.shape)
    span = _sat(days * DAY_S * unit)                           # the span saturates, then the bound does
    exact = e.astype(object) + (span if first else -span)      # Python integers: no wrap-around
    bound = np.maximum(np.minimum(exact, I64_MAX), I64_MIN).astype(np.int64)
    return t < bound if first else t > bound


def _per_user(user, ts, largest):
    """the least (or largest) timestamp of each row's user"""
    order = np.lexsort((ts, user))
    u, t = user[order], ts[order]
    starts = np.concatenate([[True], u[1:] != u[:-1]])
    ends = np.concatenate([u[1:] != u[:-1], [True]])
    group = np.cumsum(starts) - 1                               # number of the user among the sorted rows
    out = np.empty_like(ts)
    out[order] = t[np.flatnonzero(ends if largest else starts)][group]
    return out


def keep_mask(name, args, log):
    args = dict(args)
    n = len(next(iter(log.values())))
    if n == 0:
        return np.zeros(0, dtype=bool)
    if name == "filter_by_min_count":
        group = np.asarray(log[args.get("group_by", "user_idx")], dtype=np.int64)
        values, inverse, counts = np.unique(group, return_inverse=True, return_counts=True)
        return counts[inverse] >= args["num_entries"]
    if name == "filter_out_low_ratings":
        with np.errstate(invalid="ignore"):
            return np.asarray(log[args.get("rating_column", "relevance")], dtype=np.float64) >= np.float64(args["value"])
    if name == "take_num_user_interactions":
        user = np.asarray(log[args.get("user_col", "user_idx")], dtype=np.int64)
        ts = np.asarray(log[args.get("date_col", "timestamp")])
        item_col = args.get("item_col", "item_idx")
        item = None if item_col is None else np.asarray(log[item_col], dtype=np.int64)
        pos, count = _order_in_user(user, ts, item)
        k = args.get("num_interactions", 10)
        return pos < k if args.get("first", True) else count - 1 - pos < k
    if name == "take_num_days_of_user_hist":
        user = np.asarray(log[args.get("user_col", "user_idx")], dtype=np.int64)
        ts = np.asarray(log[args.get("date_col", "timestamp")])
        first = args.get("first", True)
        return _days_mask(ts, _per_user(user, ts, largest=not first), args.get("days", 10), first)
    if name == "take_num_days_of_global_hist":
        ts = np.asarray(log[args.get("date_column", "timestamp")])
        first = args.get("first", True)
        return _days_mask(ts, ts.min() if first else ts.max(), args["duration_days"], first)
    if name == "take_time_period":
        ts = np.asarray(log[args.get("date_column", "timestamp")])
        keep = np.ones(n, dtype=bool)
        if args.get("start_date") is not None:
            keep &= _at_or_after(ts, args["start_date"])
        if args.get("end_date") is not None:
            keep &= ~_at_or_after(ts, args["end_date"])
        return keep
    raise ValueError(name)


def keep_rows(name, args, log):
    return np.flatnonzero(keep_mask(name, args, log)).astype(np.int64)


class DictIndexer:
    """The Indexer with Python dicts: labels = distinct ids ascending; unseen ids are appended ascending at transform."""

    def __init__(self):
        self.labels = {"user": [], "item": []}
        self.index = {"user": {}, "item": {}}

    def fit(self, user_ids, item_ids):
        for entity, ids in (("user", user_ids), ("item", item_ids)):
            self.labels[entity] = sorted({int(v) for v in ids})
            self.index[entity] = {v: i for i, v in enumerate(self.labels[entity])}

    def transform(self, entity, ids):
        new = sorted({int(v) for v in ids} - set(self.index[entity]))
        for v in new:
            self.index[entity][v] = len(self.labels[entity])
            self.labels[entity].append(v)
        return np.array([self.index[entity][int(v)] for v in ids], dtype=np.int32)

    def inverse_transform(self, entity, idx):
        if any(not 0 <= int(j) < len(self.labels[entity]) for j in idx):
            raise ValueError("index outside the labels")
        return np.array([self.labels[entity][int(j)] for j in idx], dtype=np.int64)


# ----------------------------------------------------------------------------------------------------------
# logs
# ----------------------------------------------------------------------------------------------------------
def golden_log(case_log):
    """a log of filters_known_answers.json as numpy columns (only the columns the case gives)"""
    out = {}
    for name, values in case_log.items():
        if name == "timestamp_kind":
            continue
        if name == "timestamp":
            out[name] = np.array(values, dtype="datetime64[ns]") if case_log.get("timestamp_kind") == "datetime" else \
                np.array(values, dtype=np.int64)
        elif name in ("relevance", "rel"):
            out[name] = np.array(values, dtype=np.float64)
        else:
            out[name] = np.array(values, dtype=np.int64)
    return out


def golden_args(args):
    out = dict(args)
    for k, v in out.items():
        if isinstance(v, dict) and "datetime" in v:
            out[k] = datetime.fromisoformat(v["datetime"])
    return out
