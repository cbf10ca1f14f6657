"""Train/test splitters of replay/splitters on the GPU: UserSplitter, DateSplitter, RandomSplitter, NewUsersSplitter,
ColdUserRandomSplitter and k_folds, with the reference's constructor signatures, defaults, `_init_args`, `__str__` and
ValueErrors.  What the reference does with Spark window passes (row_number() over every user's history, distinct + join
for the cold filters) is a ranking inside each user, a row predicate and a stable compaction here -- csrc/split.hip,
integer work throughout, deterministic.

`split(log) -> (train, test)` returns the kind it was given: a pandas DataFrame (index reset), a pyarrow Table /
RecordBatch (a sequence of batches comes back as a Table) or a dict of device tensors.  Every column is carried along
and rows keep their input order (the reference guarantees none).  `split_indices(log) -> (train_rows, test_rows)`
returns the two ascending int64 device tensors for callers that hold their own columns.  Spark input: to_pandas first.
Importing this module and constructing splitters needs no GPU; split() does.

Where this deviates from the reference, on purpose:
  * ties.  `row_number().over(partitionBy(user).orderBy(ts.desc()))` leaves rows of equal timestamp to Spark; here,
    of equal timestamps the LATER input row is the more recent one (rank by key descending, row index descending);
  * random numbers.  Spark's rand(seed) and randomSplit cannot be reproduced.  The draws here are the project's
    counter-based ones: for element x (an input row index or a user id) h(x) = _mix64(_mix64(seed) ^ x) and
    u(x) = _u01(h(x)) (data.py); seed=None means 0.  RandomSplitter: row i is test iff u(i) >= 1 - test_size
    (Bernoulli like randomSplit, not exact-size); ColdUserRandomSplitter: user v and all its rows are test iff
    u(v) >= 1 - test_size; UserSplitter(shuffle=True) and k_folds rank a user's rows by h(row) (as an unsigned number)
    in place of the timestamp; user_test_size picks the users with the smallest h(user), ties by user id ascending;
  * DateSplitter with a float test_start outside (0, 1) raises ValueError (the reference fails with an IndexError);
    the other forms of test_start (int unix seconds, datetime, "yyyy-mm-dd"; a naive datetime is UTC) are compared
    exactly against the log's own timestamp dtype: datetime columns as instants, integer and float columns as unix
    seconds;
  * ids are dense non-negative indices (they index count arrays and bitmaps) and are range-checked before any launch;
  * argument checks that the reference makes at split time (item_test_size, DateSplitter's fraction) are made at
    construction as well."""
from __future__ import annotations

import calendar
import math
import numbers
from datetime import datetime, timezone
from typing import Optional, Union

import numpy as np
import torch

from . import _native as N
from . import data as D
from ._device import Engine, Ws
from ._log import _Log, dense_ids, float_column

__all__ = ["Splitter", "UserSplitter", "DateSplitter", "RandomSplitter", "NewUsersSplitter", "ColdUserRandomSplitter",
           "k_folds"]

_U64 = (1 << 64) - 1


def _seed64(seed: Optional[int]) -> int:
    return (0 if seed is None else int(seed)) & _U64


def _is_int(x) -> bool:
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def _check_test_size(test_size) -> None:
    if not 0 <= test_size <= 1:          # NaN fails too
        raise ValueError("test_size must be 0 to 1")


def _item_rule(item_test_size) -> int:
    if 0 <= item_test_size < 1.0:
        return N.SPLIT_PROPORTION
    if item_test_size >= 1 and _is_int(item_test_size):
        return N.SPLIT_QUANTITY
    raise ValueError(f"`test_size` value must be [0, 1) or a positive integer; test_size={item_test_size}")


def _instant_ns(test_start) -> int:
    """int unix seconds, datetime (naive = UTC) or "yyyy-mm-dd" -> nanoseconds since the epoch, exactly."""
    if _is_int(test_start):
        return int(test_start) * 10 ** 9
    if isinstance(test_start, datetime):
        dt = test_start if test_start.tzinfo is None else test_start.astimezone(timezone.utc)
        return calendar.timegm(dt.utctimetuple()) * 10 ** 9 + dt.microsecond * 1000
    if isinstance(test_start, str):
        return int(np.datetime64(test_start).astype("datetime64[ns]").astype(np.int64))
    raise ValueError(f"test_start must be a datetime, float, str or int, got {type(test_start)}")


def _threshold_key(test_start, ts_kind: str) -> int:
    """The least timestamp_key k of the log's timestamp dtype with value(k) >= test_start."""
    ns = _instant_ns(test_start)
    if ts_kind == "datetime":
        return ns
    if ts_kind == "int":
        return -(-ns // 10 ** 9)
    return int(D.timestamp_key(np.array([ns / 10 ** 9], dtype=np.float64))[0])


class _Run(Engine):
    """One split on the device: the range-checked id columns and the calls into csrc/split.hip."""

    def __init__(self, log: _Log, user_col: str, item_col: Optional[str], need_items: bool):
        self.log, self.n = log, log.n
        if self.n >= 1 << 31:
            raise ValueError(f"a log of {self.n} rows is beyond the splitters' 2^31 - 1")
        if need_items and item_col is None:
            log.ids(user_col)                            # a bad user column is reported first, as it always was
            raise ValueError("drop_cold_items needs an item column")
        ids = dense_ids(log, [user_col] + ([item_col] if need_items else []), "user_idx / item_idx")
        (self.u, self.n_users), (self.i, self.n_items) = ids[0], ids[1] if need_items else (None, 1)
        super().__init__(log.device)

    def rank(self, key, shuffle: bool, seed: int):
        """(rank int32[n], count int32[n_users], n_present int64[1]) -- cqlrec_split_rank"""
        rank, count = self._empty(self.n, torch.int32), self._empty(self.n_users, torch.int32)
        present = self._empty(1, torch.int64)
        self.call("split_rank", self.u, key, self.n, self.n_users, int(shuffle), seed, Ws(self.n, self.n_users), rank, count,
                  present)
        return rank, count, present

    def kth_key(self, key, m: int):
        out = self._empty(1, torch.int64)
        self.call("split_kth_key", key, self.n, int(m), Ws(self.n), out)
        return out

    def new_users(self, key, test_size: float):
        start, thr = self._empty(self.n_users, torch.int64), self._empty(1, torch.int64)
        self.call("split_new_users", self.u, key, self.n, self.n_users, float(test_size), Ws(self.n_users), start, thr)
        return start, thr

    def pick_users(self, count, seed: int, n_pick: int):
        out = self._empty(self.n_users, torch.uint8)
        self.call("split_pick_users", count, self.n_users, seed, int(n_pick), Ws(self.n_users), out)
        return out

    def classify(self, rule: int, key=None, rank=None, count=None, test_user=None, user_start=None, threshold=None,
                 n: int = 0, fold: int = 0, frac: float = 0.0, seed: int = 0):
        is_train, is_test = self._empty(self.n, torch.uint8), self._empty(self.n, torch.uint8)
        self.call("split_classify", rule, self.u, key, rank, count, test_user, user_start, threshold, self.n, int(n),
                  int(fold), float(frac), seed, is_train, is_test)
        return is_train, is_test

    def filter_test(self, is_train, is_test, cold_users: bool, cold_items: bool, zero_rel: bool) -> None:
        if not (cold_users or cold_items or zero_rel):
            return
        if zero_rel and "relevance" not in self.log.names:
            raise ValueError("log has no column relevance")
        rel = float_column(self.log, "relevance") if zero_rel else None
        self.call("split_filter_test", self.u, self.i, rel, is_train, self.n, self.n_users, self.n_items, int(cold_users),
                  int(cold_items), int(zero_rel), Ws(self.n_users, self.n_items), is_test)

    def compact(self, is_train, is_test):
        tr, te, counts = self._empty(self.n, torch.int64), self._empty(self.n, torch.int64), self._empty(2, torch.int64)
        self.call("split_compact", is_train, is_test, self.n, Ws(self.n), tr, te, counts)
        n_tr, n_te = counts.cpu().tolist()                   # the one device-to-host sync of the split proper
        return tr[:n_tr], te[:n_te]


def _no_rows(log: _Log):
    e = torch.empty(0, dtype=torch.int64, device=log.device)
    return e, e.clone()


# ----------------------------------------------------------------------------------------------------------
# the splitters
# ----------------------------------------------------------------------------------------------------------
# pylint: disable=too-few-public-methods
class Splitter:
    """Base class (replay/splitters/base_splitter.py)."""

    _init_arg_names = ["drop_cold_users", "drop_cold_items", "drop_zero_rel_in_test", "user_col", "item_col", "date_col"]

    # pylint: disable=too-many-arguments
    def __init__(self, drop_cold_items: bool, drop_cold_users: bool, drop_zero_rel_in_test: bool,
                 user_col: str = "user_idx", item_col: Optional[str] = "item_idx",
                 date_col: Optional[str] = "timestamp"):
        self.drop_cold_users = drop_cold_users
        self.drop_cold_items = drop_cold_items
        self.drop_zero_rel_in_test = drop_zero_rel_in_test
        self.user_col = user_col
        self.item_col = item_col
        self.date_col = date_col

    @property
    def _init_args(self):
        return {name: getattr(self, name) for name in self._init_arg_names}

    def __str__(self):
        return type(self).__name__

    def _core_split(self, run: _Run):
        """-> (is_train, is_test): one byte per row each, before the drop filters"""
        raise NotImplementedError

    def _indices(self, log: _Log):
        if log.n == 0:
            return _no_rows(log)
        run = _Run(log, self.user_col, self.item_col, bool(self.drop_cold_items))
        is_train, is_test = self._core_split(run)
        run.filter_test(is_train, is_test, bool(self.drop_cold_users), bool(self.drop_cold_items),
                        bool(self.drop_zero_rel_in_test))
        return run.compact(is_train, is_test)

    def split_indices(self, log):
        """(train_rows, test_rows): ascending int64 device tensors of input row indices."""
        return self._indices(_Log(log))

    def split(self, log):
        """Splits `log` into (train, test) of the kind it came as; all columns carried, input row order kept."""
        lg = _Log(log)
        train_rows, test_rows = self._indices(lg)
        return lg.take(train_rows), lg.take(test_rows)


class UserSplitter(Splitter):
    """Split inside each user's history: the last (or, with `shuffle`, random) `item_test_size` rows or fraction of rows
    of every user -- or of `user_test_size` randomly chosen users -- are test
    (replay/splitters/user_log_splitter.py)."""

    _init_arg_names = ["item_test_size", "user_test_size", "shuffle", "drop_cold_items", "drop_cold_users",
                       "drop_zero_rel_in_test", "seed", "user_col", "item_col", "date_col"]

    # pylint: disable=too-many-arguments
    def __init__(self, item_test_size: Union[float, int] = 1, user_test_size: Optional[Union[float, int]] = None,
                 shuffle=False, drop_cold_items: bool = False, drop_cold_users: bool = False,
                 drop_zero_rel_in_test: bool = True, seed: Optional[int] = None, user_col: str = "user_idx",
                 item_col: Optional[str] = "item_idx", date_col: Optional[str] = "timestamp"):
        super().__init__(drop_cold_items=drop_cold_items, drop_cold_users=drop_cold_users,
                         drop_zero_rel_in_test=drop_zero_rel_in_test, user_col=user_col, item_col=item_col,
                         date_col=date_col)
        _item_rule(item_test_size)
        self.item_test_size = item_test_size
        self.user_test_size = user_test_size
        self.shuffle = shuffle
        self.seed = seed

    def _test_user_count(self, user_count: int) -> Optional[int]:
        """users to put into test (None: all), as _get_test_users validates and counts them"""
        size = self.user_test_size
        if size is None:
            return None
        if _is_int(size):
            if 1 <= size < user_count:
                return int(size)
        elif 1 > size > 0:
            return int(math.floor(user_count * size))      # rows with _row_num <= user_count * size
        raise ValueError(f"Invalid value for user_test_size: {size}")

    def _core_split(self, run: _Run):
        rule = _item_rule(self.item_test_size)
        seed = _seed64(self.seed)
        key = None if self.shuffle else run.log.key(self.date_col)
        rank, count, present = run.rank(key, bool(self.shuffle), seed)
        test_user = None
        if self.user_test_size is not None:
            n_pick = self._test_user_count(int(present.item()))         # argument validation: one small sync
            test_user = run.pick_users(count, seed, n_pick)
        if rule == N.SPLIT_QUANTITY:
            return run.classify(N.SPLIT_QUANTITY, rank=rank, test_user=test_user, n=int(self.item_test_size))
        return run.classify(N.SPLIT_PROPORTION, rank=rank, count=count, test_user=test_user, frac=float(self.item_test_size))


class DateSplitter(Splitter):
    """Split by date: rows at or after `test_start` are test (replay/splitters/log_splitter.py).  A float test_start is
    the test fraction: the threshold is the m-th smallest timestamp, m = int(n_rows * (1 - f)) + 1."""

    _init_arg_names = ["test_start", "drop_cold_users", "drop_cold_items", "drop_zero_rel_in_test", "user_col",
                       "item_col", "date_col"]

    # pylint: disable=too-many-arguments
    def __init__(self, test_start: Union[datetime, float, str, int], drop_cold_items: bool = False,
                 drop_cold_users: bool = False, drop_zero_rel_in_test: bool = True, user_col: str = "user_idx",
                 item_col: Optional[str] = "item_idx", date_col: Optional[str] = "timestamp"):
        super().__init__(drop_cold_items=drop_cold_items, drop_cold_users=drop_cold_users,
                         drop_zero_rel_in_test=drop_zero_rel_in_test, user_col=user_col, item_col=item_col,
                         date_col=date_col)
        self._check(test_start)
        self.test_start = test_start

    @staticmethod
    def _check(test_start) -> None:
        if isinstance(test_start, float):
            if not 0 < test_start < 1:
                raise ValueError(f"a float test_start is the test fraction and must be in (0, 1); got {test_start}")
        else:
            _instant_ns(test_start)

    def _core_split(self, run: _Run):
        self._check(self.test_start)
        key = run.log.key(self.date_col)
        if isinstance(self.test_start, float):
            m = int(run.n * (1 - self.test_start)) + 1
            if m > run.n:
                raise ValueError(f"test_start={self.test_start} leaves no test row in a log of {run.n} rows")
            thr = run.kth_key(key, m)
        else:
            thr = torch.tensor([_threshold_key(self.test_start, run.log.ts_kind)], dtype=torch.int64,
                                   device=run.dev)
        return run.classify(N.SPLIT_DATE, key=key, threshold=thr)


class RandomSplitter(Splitter):
    """Assign rows to train and test at random: row i is test iff u(i) >= 1 - test_size
    (replay/splitters/log_splitter.py; the draws are this project's, see the module docstring)."""

    _init_arg_names = ["test_size", "drop_cold_items", "drop_cold_users", "drop_zero_rel_in_test", "seed", "user_col",
                       "item_col", "date_col"]

    # pylint: disable=too-many-arguments
    def __init__(self, test_size: float, drop_cold_items: bool = False, drop_cold_users: bool = False,
                 drop_zero_rel_in_test: bool = True, seed: Optional[int] = None, user_col: str = "user_idx",
                 item_col: Optional[str] = "item_idx", date_col: Optional[str] = "timestamp"):
        super().__init__(drop_cold_items=drop_cold_items, drop_cold_users=drop_cold_users,
                         drop_zero_rel_in_test=drop_zero_rel_in_test, user_col=user_col, item_col=item_col,
                         date_col=date_col)
        self.seed = seed
        self.test_size = test_size
        _check_test_size(test_size)

    def _core_split(self, run: _Run):
        _check_test_size(self.test_size)
        return run.classify(N.SPLIT_RANDOM_ROW, frac=1 - self.test_size, seed=_seed64(self.seed))


class NewUsersSplitter(Splitter):
    """Only new users go to test: the threshold is the largest user start date dt such that the users starting at or
    after dt are at least test_size of all users; train is the rows before it, test is ALL rows of the users who start
    at or after it (rows of older users from the threshold on are in neither part)
    (replay/splitters/log_splitter.py)."""

    _init_arg_names = ["test_size", "drop_cold_items", "drop_zero_rel_in_test", "user_col", "item_col", "date_col"]

    # pylint: disable=too-many-arguments
    def __init__(self, test_size: float, drop_cold_items: bool = False, drop_zero_rel_in_test: bool = True,
                 user_col: str = "user_idx", item_col: Optional[str] = "item_idx",
                 date_col: Optional[str] = "timestamp"):
        super().__init__(drop_cold_items=drop_cold_items, drop_cold_users=False,
                         drop_zero_rel_in_test=drop_zero_rel_in_test, user_col=user_col, item_col=item_col,
                         date_col=date_col)
        self.test_size = test_size
        _check_test_size(test_size)

    def _core_split(self, run: _Run):
        _check_test_size(self.test_size)
        key = run.log.key(self.date_col)
        start, thr = run.new_users(key, self.test_size)
        return run.classify(N.SPLIT_NEW_USERS, key=key, user_start=start, threshold=thr)


class ColdUserRandomSplitter(Splitter):
    """Test is all rows of randomly chosen users: user v is a test user iff u(v) >= 1 - test_size
    (replay/splitters/log_splitter.py; the draws are this project's, see the module docstring)."""

    _init_arg_names = ["test_size", "drop_cold_items", "drop_cold_users", "drop_zero_rel_in_test", "seed", "user_col",
                       "item_col", "date_col"]

    # pylint: disable=too-many-arguments
    def __init__(self, test_size: float, drop_cold_items: bool = False, drop_cold_users: bool = False,
                 drop_zero_rel_in_test: bool = True, seed: Optional[int] = None, user_col: str = "user_idx",
                 item_col: Optional[str] = "item_idx", date_col: Optional[str] = "timestamp"):
        super().__init__(drop_cold_items=drop_cold_items, drop_cold_users=drop_cold_users,
                         drop_zero_rel_in_test=drop_zero_rel_in_test, user_col=user_col, item_col=item_col,
                         date_col=date_col)
        self.test_size = test_size
        self.seed = seed
        _check_test_size(test_size)

    def _core_split(self, run: _Run):
        _check_test_size(self.test_size)
        return run.classify(N.SPLIT_RANDOM_USER, frac=1 - self.test_size, seed=_seed64(self.seed))


def k_folds(log, n_folds: Optional[int] = 5, seed: Optional[int] = None, splitter: Optional[str] = "user",
            user_col: str = "user_idx"):
    """Splits the log inside each user into folds at random: a row goes to fold `rank % n_folds`, rank being the row's
    number inside its user under the shuffle key h(row) (replay/splitters/user_log_splitter.py:307-338).  Yields
    (train, test) per fold, of the kind `log` came as."""
    if splitter not in {"user"}:
        raise ValueError(f"Wrong splitter parameter: {splitter}")
    if not _is_int(n_folds) or n_folds < 1:
        raise ValueError(f"n_folds must be a positive integer, got {n_folds}")
    lg = _Log(log)
    if lg.n == 0:
        for _ in range(n_folds):
            train_rows, test_rows = _no_rows(lg)
            yield lg.take(train_rows), lg.take(test_rows)
        return
    run = _Run(lg, user_col, None, False)
    rank, _, _ = run.rank(None, True, _seed64(seed))
    for fold in range(n_folds):
        train_rows, test_rows = run.compact(*run.classify(N.SPLIT_FOLD, rank=rank, n=n_folds, fold=fold))
        yield lg.take(train_rows), lg.take(test_rows)
