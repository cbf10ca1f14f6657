"""Plain numpy implementation of the splitter semantics of replay_cql_amd/splitters.py, written from their definition
(not from the device code): the yardstick of tests/test_gpu_splitters.py, checked itself against the known answers
of tests/golden/splitters_known_answers.json by tests/test_split_reference_cpu.py.

A log is a dict of numpy columns: user_idx, item_idx, relevance, timestamp (int64, float64 or datetime64).
`split_rows(name, args, log)` -> (train_rows, test_rows), ascending int64 input row indices."""
from __future__ import annotations

import math
from datetime import datetime
from fractions import Fraction

import numpy as np

_GOLD, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix64(z):
    """splitmix64 step on uint64 arrays (wrapping arithmetic)"""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = z + _GOLD
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def draw(seed, x):
    """h(x) = mix64(mix64(seed) ^ x) for element ids x; seed None = 0"""
    s = np.uint64((0 if seed is None else int(seed)) & ((1 << 64) - 1))
    return mix64(mix64(s)[0] ^ np.asarray(x).astype(np.uint64))


def u01(h):
    return ((h >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / (1 << 53))


def rank_in_user(user, key):
    """1-based row number inside the user by (key descending, input row descending) + rows per user id"""
    user = np.asarray(user, dtype=np.int64)
    n = len(user)
    counts = np.bincount(user, minlength=int(user.max()) + 1 if n else 0).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(counts) else counts
    order = np.lexsort((np.arange(n), key, user))          # ascending (key, row) inside the user ...
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    return counts[user] - (pos - starts[user]), counts      # ... read backwards


def _shuffle_key(n, seed):
    return draw(seed, np.arange(n))


def _test_users(user, user_test_size, seed):
    present = np.unique(user)
    if user_test_size is None:
        return present
    user_count = len(present)
    if isinstance(user_test_size, (int, np.integer)) and not isinstance(user_test_size, bool):
        if not 1 <= user_test_size < user_count:
            raise ValueError("user_test_size")
        n_pick = int(user_test_size)
    else:
        if not 0 < user_test_size < 1:
            raise ValueError("user_test_size")
        n_pick = sum(1 for r in range(1, user_count + 1) if r <= user_count * user_test_size)
    h = draw(seed, present)
    return present[np.lexsort((present, h))[:n_pick]]


def _seconds(test_start) -> Fraction:
    if isinstance(test_start, str):
        return Fraction(int(np.datetime64(test_start).astype("datetime64[s]").astype(np.int64)))
    if isinstance(test_start, datetime):
        whole = np.datetime64(test_start.replace(microsecond=0)).astype("datetime64[s]").astype(np.int64)
        return Fraction(int(whole)) + Fraction(test_start.microsecond, 10 ** 6)
    return Fraction(int(test_start))


def core_masks(name, args, log):
    """(is_train, is_test) boolean masks BEFORE the drop filters"""
    user = np.asarray(log["user_idx"], dtype=np.int64)
    n = len(user)
    ts = np.asarray(log["timestamp"]) if "timestamp" in log else None
    seed = args.get("seed")
    if name == "UserSplitter":
        size = args.get("item_test_size", 1)
        key = _shuffle_key(n, seed) if args.get("shuffle", False) else ts
        rank, counts = rank_in_user(user, key)
        in_test_user = np.isin(user, _test_users(user, args.get("user_test_size"), seed))
        if 0 <= size < 1.0:
            test = (rank.astype(np.float64) / counts[user].astype(np.float64) <= size) & in_test_user
        elif size >= 1 and isinstance(size, (int, np.integer)):
            test = (rank <= size) & in_test_user
        else:
            raise ValueError("item_test_size")
        return ~test, test
    if name == "DateSplitter":
        start = args["test_start"]
        if isinstance(start, float):
            if not 0 < start < 1:
                raise ValueError("test_start")
            m = int(n * (1 - start)) + 1
            test = ts >= np.sort(ts)[m - 1]
        elif ts.dtype.kind == "M":
            sec = _seconds(start)
            test = ts.astype("datetime64[ns]").astype(np.int64).astype(object) >= sec * 10 ** 9
            test = test.astype(bool)
        elif ts.dtype.kind in "iu":
            test = ts >= math.ceil(_seconds(start))
        else:
            test = ts >= float(_seconds(start))
        return ~test, test
    if name == "RandomSplitter":
        test = u01(draw(seed, np.arange(n))) >= 1 - args["test_size"]
        return ~test, test
    if name == "ColdUserRandomSplitter":
        test = u01(draw(seed, user)) >= 1 - args["test_size"]
        return ~test, test
    if name == "NewUsersSplitter":
        present = np.unique(user)
        start_of = {int(v): ts[user == v].min() for v in present} if len(present) < 64 else None
        if start_of is None:
            order = np.lexsort((ts, user))
            first = np.concatenate([[True], user[order][1:] != user[order][:-1]])
            start_of = dict(zip(user[order][first].tolist(), ts[order][first]))
        starts = np.array([start_of[int(v)] for v in present])
        total = len(present)
        threshold = None
        for dt in np.unique(starts):                       # ascending: the last one that qualifies is the largest
            if float((starts >= dt).sum()) >= total * args["test_size"]:
                threshold = dt
        train = ts < threshold
        test = np.array([start_of[int(v)] >= threshold for v in user], dtype=bool)
        return train, test
    raise ValueError(name)


def apply_filters(log, train, test, drop_cold_users=False, drop_cold_items=False, drop_zero_rel_in_test=True):
    user, item = np.asarray(log["user_idx"]), np.asarray(log["item_idx"])
    test = test.copy()
    if drop_cold_items:
        test &= np.isin(item, item[train])
    if drop_cold_users:
        test &= np.isin(user, user[train])
    if drop_zero_rel_in_test:
        test &= np.asarray(log["relevance"], dtype=np.float64) > 0.0
    return test


_DEFAULT_ZERO_REL = True


def split_rows(name, args, log):
    args = dict(args)
    flags = {"drop_cold_users": args.pop("drop_cold_users", False), "drop_cold_items": args.pop("drop_cold_items", False),
             "drop_zero_rel_in_test": args.pop("drop_zero_rel_in_test", _DEFAULT_ZERO_REL)}
    if len(log["user_idx"]) == 0:
        e = np.zeros(0, dtype=np.int64)
        return e, e
    train, test = core_masks(name, args, log)
    test = apply_filters(log, train, test, **flags)
    return np.flatnonzero(train).astype(np.int64), np.flatnonzero(test).astype(np.int64)


def fold_rows(log, n_folds, seed):
    """k_folds: per fold (train_rows, test_rows); fold of a row = rank % n_folds under the shuffle key"""
    user = np.asarray(log["user_idx"], dtype=np.int64)
    rank, _ = rank_in_user(user, _shuffle_key(len(user), seed))
    out = []
    for f in range(n_folds):
        test = rank % n_folds == f
        out.append((np.flatnonzero(~test).astype(np.int64), np.flatnonzero(test).astype(np.int64)))
    return out


# ----------------------------------------------------------------------------------------------------------
# logs
# ----------------------------------------------------------------------------------------------------------
def golden_log(case_log):
    """a log of splitters_known_answers.json as numpy columns"""
    ts = case_log["timestamp"]
    ts = np.array(ts, dtype="datetime64[ns]") if case_log["timestamp_kind"] == "datetime" else np.array(ts, dtype=np.int64)
    return {"user_idx": np.array(case_log["user_idx"], dtype=np.int64),
            "item_idx": np.array(case_log["item_idx"], dtype=np.int64),
            "relevance": np.array(case_log["relevance"], dtype=np.float64), "timestamp": ts}


def golden_args(args):
    out = dict(args)
    if isinstance(out.get("test_start"), dict):
        out["test_start"] = datetime.fromisoformat(out["test_start"]["datetime"])
    return out


DAY0 = 1567296000          # 2019-09-01T00:00:00Z


def edge_log(n_rows=70001, n_users=3000, big=5000, n_days=50, ts_kind="int", seed=20191):
    """A log that hits the edges: a row count that is no multiple of any block size, user slots without rows (every
    97th id), one user with `big` rows, users of 1 and of 2 rows, n_days distinct timestamps (ties everywhere), rows
    of relevance <= 0, items that only occur on the last day (test-only under a date split); rows in random order.
    ts_kind: int (unix seconds), float (negative and fractional) or datetime (datetime64[ns])."""
    rng = np.random.default_rng(seed)
    ones, twos = np.arange(10, 20), np.arange(20, 30)
    fixed = np.concatenate([np.full(big, 7), ones, np.repeat(twos, 2), [n_users - 1]])
    free = np.array([v for v in range(n_users) if v % 97 != 0 and v != 7 and not 10 <= v < 30])
    user = np.concatenate([fixed, rng.choice(free, n_rows - len(fixed))])
    rng.shuffle(user)
    day = rng.integers(0, n_days, n_rows)
    item = rng.integers(0, 500, n_rows)
    last = np.flatnonzero(day == n_days - 1)[:60]
    item[last] = 500 + np.arange(len(last))
    rel = rng.choice(np.array([-1.0, 0.0, 0.5, 1.0, 2.0]), n_rows)
    if ts_kind == "int":
        ts = (DAY0 + day * 86400).astype(np.int64)
    elif ts_kind == "float":
        ts = (day - n_days // 2).astype(np.float64) * 0.37
    else:
        ts = (DAY0 + day * 86400).astype("datetime64[s]").astype("datetime64[ns]")
    return {"user_idx": user.astype(np.int64), "item_idx": item.astype(np.int64), "relevance": rel, "timestamp": ts}
