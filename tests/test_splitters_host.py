"""replay_cql_amd.splitters without a GPU: the module imports, the classes carry the reference's constructor signatures,
defaults, `_init_args`, `__str__` and ValueErrors, and the host-only side of the new entry points (workspace queries,
argument validation before any launch) behaves."""
import inspect
from datetime import datetime

import numpy as np
import pytest

import replay_cql_amd
from replay_cql_amd import _native as N
from replay_cql_amd import build as B
from replay_cql_amd import data as D
from replay_cql_amd import splitters as S

BASE = dict(user_col="user_idx", item_col="item_idx", date_col="timestamp")


def test_package_exports_the_splitters():
    for name in ("UserSplitter", "DateSplitter", "RandomSplitter", "NewUsersSplitter", "ColdUserRandomSplitter", "k_folds"):
        assert getattr(replay_cql_amd, name) is getattr(S, name)
    assert inspect.isgeneratorfunction(S.k_folds)


def test_signatures_and_defaults_are_the_references():
    def params(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]

    E = inspect.Parameter.empty
    tail = [("user_col", "user_idx"), ("item_col", "item_idx"), ("date_col", "timestamp")]
    assert params(S.UserSplitter) == [("item_test_size", 1), ("user_test_size", None), ("shuffle", False),
                                      ("drop_cold_items", False), ("drop_cold_users", False),
                                      ("drop_zero_rel_in_test", True), ("seed", None)] + tail
    assert params(S.DateSplitter) == [("test_start", E), ("drop_cold_items", False), ("drop_cold_users", False),
                                      ("drop_zero_rel_in_test", True)] + tail
    for cls in (S.RandomSplitter, S.ColdUserRandomSplitter):
        assert params(cls) == [("test_size", E), ("drop_cold_items", False), ("drop_cold_users", False),
                               ("drop_zero_rel_in_test", True), ("seed", None)] + tail
    assert params(S.NewUsersSplitter) == [("test_size", E), ("drop_cold_items", False),
                                          ("drop_zero_rel_in_test", True)] + tail
    assert [(p.name, p.default) for p in inspect.signature(S.k_folds).parameters.values()] == [
        ("log", E), ("n_folds", 5), ("seed", None), ("splitter", "user"), ("user_col", "user_idx")]


@pytest.mark.parametrize("splitter,expected", [
    (S.UserSplitter(item_test_size=0.3, user_test_size=4, shuffle=True, drop_cold_items=True, seed=9, user_col="u"),
     dict(item_test_size=0.3, user_test_size=4, shuffle=True, drop_cold_items=True, drop_cold_users=False,
          drop_zero_rel_in_test=True, seed=9, user_col="u", item_col="item_idx", date_col="timestamp")),
    (S.DateSplitter("2020-01-02", drop_cold_users=True, date_col="ts"),
     dict(test_start="2020-01-02", drop_cold_users=True, drop_cold_items=False, drop_zero_rel_in_test=True,
          user_col="user_idx", item_col="item_idx", date_col="ts")),
    (S.RandomSplitter(0.2, seed=3, drop_zero_rel_in_test=False),
     dict(test_size=0.2, drop_cold_items=False, drop_cold_users=False, drop_zero_rel_in_test=False, seed=3, **BASE)),
    (S.NewUsersSplitter(0.1, drop_cold_items=True),
     dict(test_size=0.1, drop_cold_items=True, drop_zero_rel_in_test=True, **BASE)),
    (S.ColdUserRandomSplitter(0.5, item_col=None),
     dict(test_size=0.5, drop_cold_items=False, drop_cold_users=False, drop_zero_rel_in_test=True, seed=None,
          user_col="user_idx", item_col=None, date_col="timestamp")),
])
def test_init_args_round_trip(splitter, expected):
    args = splitter._init_args
    assert args == expected and list(args) == type(splitter)._init_arg_names
    again = type(splitter)(**args)
    assert again._init_args == args
    assert str(splitter) == type(splitter).__name__


def test_new_users_splitter_never_drops_cold_users():
    assert S.NewUsersSplitter(0.3).drop_cold_users is False
    assert "drop_cold_users" not in S.NewUsersSplitter(0.3)._init_args


@pytest.mark.parametrize("value", [2.0, 2.1, -1, -0.01, -50])
def test_item_test_size_outside_its_domain_raises(value):
    with pytest.raises(ValueError):
        S.UserSplitter(item_test_size=value)


@pytest.mark.parametrize("value", [0, 0.0, 0.5, 0.99, 1, 3, 1000])
def test_item_test_size_inside_its_domain(value):
    assert S.UserSplitter(item_test_size=value).item_test_size == value


@pytest.mark.parametrize("cls", [S.RandomSplitter, S.NewUsersSplitter, S.ColdUserRandomSplitter])
@pytest.mark.parametrize("value", [-1.0, 2.0, -0.01, 1.01, float("nan")])
def test_test_size_outside_0_1_raises(cls, value):
    with pytest.raises(ValueError):
        cls(value)
    assert cls(0.0).test_size == 0.0 and cls(1.0).test_size == 1.0


@pytest.mark.parametrize("value", [0.0, 1.0, -0.2, 1.5])
def test_date_splitter_fraction_outside_the_open_interval_raises(value):
    """a deliberate deviation: the reference fails with an IndexError at split time"""
    with pytest.raises(ValueError):
        S.DateSplitter(value)


def test_date_splitter_accepts_every_form_of_test_start():
    for start in (0.2, 1568505600, datetime(2019, 9, 15), "2019-09-15"):
        assert S.DateSplitter(start).test_start == start
    with pytest.raises(ValueError):
        S.DateSplitter(None)
    # one instant, three spellings, three column dtypes
    ns = 1568505600 * 10 ** 9
    assert S._instant_ns(datetime(2019, 9, 15)) == S._instant_ns("2019-09-15") == S._instant_ns(1568505600) == ns
    assert S._threshold_key("2019-09-15", "datetime") == ns
    assert S._threshold_key(datetime(2019, 9, 15, 0, 0, 0, 1), "int") == 1568505601     # the least second not before it
    assert S._threshold_key(-3, "float") == int(D.timestamp_key(np.array([-3.0]))[0])


def test_user_test_size_rule():
    s = S.UserSplitter(user_test_size=3)
    assert s._test_user_count(5) == 3
    assert S.UserSplitter(user_test_size=0.6)._test_user_count(5) == 3
    assert S.UserSplitter(user_test_size=0.3)._test_user_count(2903) == 870
    assert S.UserSplitter()._test_user_count(5) is None
    for bad in (5, 0, 1.0, 0.0, -1):
        with pytest.raises(ValueError):
            S.UserSplitter(user_test_size=bad)._test_user_count(5)


def test_k_folds_rejects_other_strategies_before_touching_the_log():
    with pytest.raises(ValueError, match="Wrong splitter"):
        next(S.k_folds(None, splitter="item"))


def test_split_entry_points_validate_on_the_host():
    B.build(verbose=False)
    lib = N.load()
    assert lib.cqlrec_split_rank_ws_bytes(1000, 10) > 1000 * 24
    assert lib.cqlrec_split_rank_ws_bytes(2000, 10) > lib.cqlrec_split_rank_ws_bytes(1000, 10)
    assert lib.cqlrec_split_kth_key_ws_bytes(1000) > 8000
    assert lib.cqlrec_split_new_users_ws_bytes(1000) > 12000
    assert lib.cqlrec_split_pick_users_ws_bytes(1000) > 24000
    assert lib.cqlrec_split_filter_test_ws_bytes(64, 33) >= 8 + 8
    assert lib.cqlrec_split_compact_ws_bytes(1000) > 0
    big = 1 << 31
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_split_rank(None, None, big, 10, 0, 0, None, 0, None, None, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_split_kth_key(None, big, 1, None, 0, None, None))
    with pytest.raises(N.CqlrecError, match="outside 1"):
        N.check(lib.cqlrec_split_kth_key(None, 10, 11, None, 0, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_split_new_users(None, None, big, 10, 0.5, None, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="test_size"):
        N.check(lib.cqlrec_split_new_users(None, None, 10, 10, 1.5, None, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_split_pick_users(None, 10, 0, 1, None, 0, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_split_classify(0, None, None, None, None, None, None, None, big, 1, 0, 0.0, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="unknown rule"):
        N.check(lib.cqlrec_split_classify(7, None, None, None, None, None, None, None, 10, 1, 0, 0.0, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_split_classify(2, None, None, None, None, None, None, None, 10, 1, 0, 0.0, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_split_filter_test(None, None, None, None, big, 1, 1, 1, 1, 1, None, 0, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_split_compact(None, None, big, None, 0, None, None, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_split_compact(None, None, 10, None, 0, None, None, None, None))
