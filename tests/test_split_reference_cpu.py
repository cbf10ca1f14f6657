"""tests/split_reference.py, the yardstick of the device splitters, reproduces every known answer the reference pins
(tests/golden/splitters_known_answers.json), draws the project's random numbers (data._mix64 / data._u01) and splits the
way the splitters are defined.  No GPU."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import split_reference as R
from replay_cql_amd import data as D

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "splitters_known_answers.json").read_text())


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_reference_reproduces_known_answers(case):
    log = R.golden_log(case["log"])
    train, test = R.split_rows(case["splitter"], R.golden_args(case["args"]), log)
    if case["train_rows"] is not None:
        assert train.tolist() == case["train_rows"]
    if case["test_rows"] is not None:
        assert test.tolist() == case["test_rows"]
    for u, c in case.get("test_rows_per_user", {}).items():
        assert int((log["user_idx"][test] == int(u)).sum()) == c


def test_fixture_states_what_it_leaves_out():
    assert "Spark" in GOLDEN["note"] and "[0, 2, 3]" in GOLDEN["note"]
    assert len(GOLDEN["cases"]) >= 12


def test_draws_are_the_projects_counter_based_numbers():
    x = np.concatenate([np.arange(1000), [2 ** 31, 2 ** 40 + 7, 2 ** 62]]).astype(np.int64)
    for seed in (0, 1, 1234, 2 ** 63 + 5):
        s = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64)
        h = D._mix64(D._mix64(s) ^ torch.as_tensor(x))
        assert np.array_equal(h.numpy().view(np.uint64), R.draw(seed, x))
        assert np.array_equal(D._u01(h).numpy(), R.u01(R.draw(seed, x)))
    assert np.array_equal(R.draw(None, x), R.draw(0, x))
    u = R.u01(R.draw(7, np.arange(200000)))
    assert 0.0 < u.min() and u.max() <= 1.0 and abs(u.mean() - 0.5) < 0.01


def test_rank_breaks_ties_by_the_later_row():
    user = np.array([0, 1, 0, 0, 1, 0])
    key = np.array([5, 5, 5, 9, 5, 5])
    rank, counts = R.rank_in_user(user, key)
    assert rank.tolist() == [4, 2, 3, 1, 1, 2] and counts.tolist() == [4, 2]
    # extreme keys: no negation anywhere
    key = np.array([np.iinfo(np.int64).min, 0, np.iinfo(np.int64).max, -1, 0, np.iinfo(np.int64).min])
    rank, _ = R.rank_in_user(user, key)
    assert rank.tolist() == [4, 2, 1, 2, 1, 3]


SMALL = R.edge_log(n_rows=4001, n_users=300, big=700, n_days=9)
CASES = [
    ("UserSplitter", {"item_test_size": 1}),
    ("UserSplitter", {"item_test_size": 0.35, "shuffle": True, "seed": 3, "user_test_size": 0.3}),
    ("UserSplitter", {"item_test_size": 3, "user_test_size": 7, "seed": 5}),
    ("DateSplitter", {"test_start": 0.2}),
    ("DateSplitter", {"test_start": R.DAY0 + 4 * 86400}),
    ("RandomSplitter", {"test_size": 0.25, "seed": 1}),
    ("ColdUserRandomSplitter", {"test_size": 0.25, "seed": 1}),
]


@pytest.mark.parametrize("name,args", CASES)
def test_train_and_test_partition_the_log_before_the_filters(name, args):
    train, test = R.core_masks(name, args, SMALL)
    assert np.array_equal(train, ~test)
    assert 0 < test.sum() < len(test)


@pytest.mark.parametrize("test_size", [0.0, 0.1, 0.5, 1.0])
def test_new_users_parts_are_disjoint_and_miss_only_old_users_late_rows(test_size):
    """NewUsersSplitter is the one splitter whose parts do not cover the log: train is the rows before the threshold, test
    all rows of the users who start at or after it, so the rows of OLDER users from the threshold on are in neither
    (the reference's first docstring example drops the row (1, 2, 40) this way)."""
    train, test = R.core_masks("NewUsersSplitter", {"test_size": test_size}, SMALL)
    assert not (train & test).any()
    user, ts = SMALL["user_idx"], SMALL["timestamp"]
    thr = ts[test].min() if test.any() else None
    assert thr is not None
    start = {int(v): ts[user == v].min() for v in np.unique(user)}
    old = np.array([start[int(v)] < thr for v in user])
    assert np.array_equal(~(train | test), old & (ts >= thr))
    assert not np.isin(user[test], user[train]).any()
    n_users, n_test_users = len(start), len(np.unique(user[test]))
    assert n_test_users >= n_users * test_size
    # the largest such threshold: starting any later would leave fewer than test_size of the users
    later = sum(1 for s in start.values() if s > thr)
    assert later < n_users * test_size or later == 0


def test_user_test_size_counts_and_errors():
    user = SMALL["user_idx"]
    n_present = len(np.unique(user))
    _, test = R.core_masks("UserSplitter", {"user_test_size": 7, "seed": 2}, SMALL)
    assert len(np.unique(user[test])) == 7
    _, test = R.core_masks("UserSplitter", {"user_test_size": 0.3, "seed": 2}, SMALL)
    assert len(np.unique(user[test])) == int(np.floor(n_present * 0.3))
    for bad in (0, n_present, 1.0, 0.0, -0.5):
        with pytest.raises(ValueError):
            R.core_masks("UserSplitter", {"user_test_size": bad}, SMALL)


def test_filters_only_touch_test():
    train, test = R.core_masks("DateSplitter", {"test_start": R.DAY0 + 8 * 86400}, SMALL)
    kept = R.apply_filters(SMALL, train, test, drop_cold_users=True, drop_cold_items=True, drop_zero_rel_in_test=True)
    assert (kept <= test).all() and kept.sum() < test.sum()
    assert (SMALL["relevance"][kept] > 0).all()
    assert np.isin(SMALL["item_idx"][kept], SMALL["item_idx"][train]).all()
    assert np.isin(SMALL["user_idx"][kept], SMALL["user_idx"][train]).all()
    assert (SMALL["item_idx"][test] >= 500).any()           # the last day's own items are cold


def test_k_folds_partition_and_balance():
    folds = R.fold_rows(SMALL, 5, seed=11)
    n = len(SMALL["user_idx"])
    assert np.array_equal(np.sort(np.concatenate([te for _, te in folds])), np.arange(n))
    per = np.stack([np.bincount(SMALL["user_idx"][te], minlength=300) for _, te in folds])
    assert (per.max(0) - per.min(0) <= 1).all()
