"""The splitters on the GPU (replay_cql_amd.splitters, csrc/split.hip) against tests/split_reference.py: the device result
is the reference's EXACTLY -- the same ascending int64 row indices -- since a split is integer work (and the one
division and the uniform draws are single IEEE double operations on both sides).

The log of most tests is split_reference.edge_log(): 70 001 rows (no multiple of a block, many blocks), 3 000 user slots
some of which have no rows, one user of 5 000 rows, users of 1 and 2 rows, 50 distinct timestamps (ties everywhere),
rows of relevance <= 0 and items that occur only in the test part of a date split."""
import json
from datetime import datetime
from pathlib import Path

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

import split_reference as R
from replay_cql_amd import splitters as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "splitters_known_answers.json").read_text())
CLASSES = {c.__name__: c for c in (S.UserSplitter, S.DateSplitter, S.RandomSplitter, S.NewUsersSplitter,
                                   S.ColdUserRandomSplitter)}
_LOGS, _DEVICE_LOGS = {}, {}


def edge(ts_kind="int"):
    if ts_kind not in _LOGS:
        _LOGS[ts_kind] = R.edge_log(ts_kind=ts_kind)
    return _LOGS[ts_kind]


def on_device(log, key=None):
    """a numpy log as a dict of device tensors (datetime64 has no torch dtype: those logs go in as pandas)"""
    if key is not None and key in _DEVICE_LOGS:
        return _DEVICE_LOGS[key]
    out = {k: torch.as_tensor(v).to(DEV) for k, v in log.items()}
    if key is not None:
        _DEVICE_LOGS[key] = out
    return out


def given(log, ts_kind):
    return pd.DataFrame(log) if ts_kind == "datetime" else on_device(log, ts_kind)


def check(name, args, log, device_log):
    want_train, want_test = R.split_rows(name, args, log)
    train, test = CLASSES[name](**args).split_indices(device_log)
    assert train.dtype == torch.int64 and test.dtype == torch.int64 and train.is_cuda and test.is_cuda
    got_train, got_test = train.cpu().numpy(), test.cpu().numpy()
    print(name, args, "train", len(got_train), "test", len(got_test))
    assert np.array_equal(got_train, want_train), (name, args)
    assert np.array_equal(got_test, want_test), (name, args)
    return got_train, got_test


def flags(i):
    """the i-th of the eight on/off combinations of the three drop flags"""
    return {"drop_cold_items": bool(i & 1), "drop_cold_users": bool(i & 2), "drop_zero_rel_in_test": bool(i & 4)}


# ---------------------------------------------------------------------------------------------------------------------
# every splitter over its parameter grid, on the edge log
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("user_test_size", [None, 7, 0.3])
def test_user_splitter_grid(user_test_size, shuffle):
    log = edge()
    dev = on_device(log, "int")
    sizes = 0
    for i, item_test_size in enumerate([1, 3, 0.1, 0.35, 0.6]):
        for j in (i, i + 3):                                   # every drop flag on and off with every size
            args = dict(item_test_size=item_test_size, user_test_size=user_test_size, shuffle=shuffle, seed=1234 + i,
                        **flags(j))
            _, test = check("UserSplitter", args, log, dev)
            sizes += len(test)
    assert sizes > 0


def test_user_splitter_all_flag_combinations_and_seeds():
    log = edge()
    dev = on_device(log, "int")
    for f in range(8):
        check("UserSplitter", dict(item_test_size=0.35, **flags(f)), log, dev)
    a = check("UserSplitter", dict(item_test_size=2, shuffle=True, seed=None, drop_zero_rel_in_test=False), log, dev)
    b = check("UserSplitter", dict(item_test_size=2, shuffle=True, seed=0, drop_zero_rel_in_test=False), log, dev)
    c = check("UserSplitter", dict(item_test_size=2, shuffle=True, seed=-7, drop_zero_rel_in_test=False), log, dev)
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1])           # seed=None means 0
    # ties go to the later row: with one test row per user, it is the LAST of the user's rows on its latest day
    _, test = check("UserSplitter", dict(drop_zero_rel_in_test=False), log, dev)
    u, t = log["user_idx"], log["timestamp"]
    assert len(test) == len(np.unique(u))
    big = np.flatnonzero(u == 7)
    assert np.intersect1d(test, big).tolist() == [big[t[big] == t[big].max()].max()]


@pytest.mark.parametrize("ts_kind", ["int", "float", "datetime"])
def test_user_splitter_timestamp_dtypes(ts_kind):
    log = edge(ts_kind)
    if ts_kind == "float":
        assert (log["timestamp"] < 0).any() and (log["timestamp"] != np.round(log["timestamp"])).any()
    for size in (1, 0.35):
        check("UserSplitter", dict(item_test_size=size, drop_cold_items=True), log, given(log, ts_kind))


@pytest.mark.parametrize("user_test_size", [0, 1.0, 0.0, 10 ** 6, -3])
def test_user_test_size_out_of_range_raises(user_test_size):
    with pytest.raises(ValueError, match="user_test_size"):
        S.UserSplitter(user_test_size=user_test_size).split_indices(on_device(edge(), "int"))


DATE_FORMS = {
    "int": [0.2, 0.5, R.DAY0 + 19 * 86400, datetime(2019, 9, 20), "2019-09-20", datetime(2019, 9, 20, 0, 0, 0, 5),
            R.DAY0 - 1, R.DAY0 + 500 * 86400],
    "float": [0.2, -3, 0, 5],
    "datetime": [0.2, R.DAY0 + 19 * 86400, datetime(2019, 9, 20), "2019-09-20", datetime(2019, 9, 20, 0, 0, 0, 5)],
}


@pytest.mark.parametrize("ts_kind", ["int", "float", "datetime"])
def test_date_splitter_forms_and_dtypes(ts_kind):
    log = edge(ts_kind)
    dev = given(log, ts_kind)
    for i, start in enumerate(DATE_FORMS[ts_kind]):
        train, test = check("DateSplitter", dict(test_start=start, **flags(i)), log, dev)
        if i == 0:
            assert 0 < len(test) < len(train)
    if ts_kind != "float":      # the three spellings of one instant split alike
        got = [check("DateSplitter", dict(test_start=s, drop_zero_rel_in_test=False), log, dev)
               for s in (R.DAY0 + 19 * 86400, datetime(2019, 9, 20), "2019-09-20")]
        assert all(np.array_equal(g[1], got[0][1]) for g in got) and len(got[0][1]) > 0
        # items that only occur on the last day are cold under a date split that cuts before it
        _, kept = check("DateSplitter", dict(test_start="2019-10-19", drop_cold_items=True, drop_zero_rel_in_test=False),
                        log, dev)
        _, every = check("DateSplitter", dict(test_start="2019-10-19", drop_zero_rel_in_test=False), log, dev)
        assert (log["item_idx"][every] >= 500).any() and not (log["item_idx"][kept] >= 500).any()


@pytest.mark.parametrize("name", ["RandomSplitter", "ColdUserRandomSplitter", "NewUsersSplitter"])
@pytest.mark.parametrize("test_size", [0.0, 0.25, 1.0])
def test_test_size_splitters_grid(name, test_size):
    log = edge()
    dev = on_device(log, "int")
    for f in range(8):
        fl = flags(f)
        if name == "NewUsersSplitter":
            if fl.pop("drop_cold_users"):
                continue
            check(name, dict(test_size=test_size, **fl), log, dev)
        else:
            check(name, dict(test_size=test_size, seed=f, **fl), log, dev)
    if name == "NewUsersSplitter":
        for ts_kind in ("float", "datetime"):
            lg = edge(ts_kind)
            check(name, dict(test_size=test_size), lg, given(lg, ts_kind))
        check(name, dict(test_size=0.1), log, dev)
    elif test_size == 0.25:
        _, test = check(name, dict(test_size=test_size, seed=99, drop_zero_rel_in_test=False), log, dev)
        share = len(test) / len(log["user_idx"]) if name == "RandomSplitter" else \
            len(np.unique(log["user_idx"][test])) / len(np.unique(log["user_idx"]))
        assert abs(share - 0.25) < 0.05                        # Bernoulli, not exact-size


# ---------------------------------------------------------------------------------------------------------------------
# known answers, kinds of input, determinism, k_folds, degenerate logs, end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_known_answers_through_the_device_path(case):
    log = R.golden_log(case["log"])
    splitter = CLASSES[case["splitter"]](**R.golden_args(case["args"]))
    train, test = splitter.split(pd.DataFrame(log))
    assert isinstance(train, pd.DataFrame) and list(train.columns) == list(log)
    frame = pd.DataFrame(log)
    if case["train_rows"] is not None:
        pd.testing.assert_frame_equal(train, frame.iloc[case["train_rows"]].reset_index(drop=True))
    if case["test_rows"] is not None:
        pd.testing.assert_frame_equal(test, frame.iloc[case["test_rows"]].reset_index(drop=True))
    for u, c in case.get("test_rows_per_user", {}).items():
        assert int((test.user_idx == int(u)).sum()) == c


def _frame():
    log = R.edge_log(n_rows=5001, n_users=400, big=600, n_days=11, ts_kind="datetime")
    frame = pd.DataFrame({"user_idx": log["user_idx"].astype(np.int32), "item_idx": log["item_idx"].astype(np.int16),
                          "timestamp": log["timestamp"], "relevance": log["relevance"].astype(np.float32)})
    frame["note"] = [f"row{i}" for i in range(len(frame))]               # an extra column, not even numeric
    frame["weight"] = np.arange(len(frame), dtype=np.float64) * 0.5
    frame.index = frame.index[::-1]                                      # an index the output must not carry
    return log, frame


def test_the_kind_that_goes_in_comes_out_with_every_column():
    log, frame = _frame()
    args = dict(item_test_size=0.35, drop_cold_items=True)
    want_train, want_test = R.split_rows("UserSplitter", args, log)
    splitter = S.UserSplitter(**args)
    # pandas
    train, test = splitter.split(frame)
    for got, rows in ((train, want_train), (test, want_test)):
        assert isinstance(got, pd.DataFrame)
        pd.testing.assert_frame_equal(got, frame.iloc[rows].reset_index(drop=True))      # values, dtypes, fresh index
    assert dict(train.dtypes) == dict(frame.dtypes) and len(test) > 0
    # Arrow: table, record batch, sequence of batches
    table = pa.Table.from_pandas(frame, preserve_index=False)
    for src, kind in ((table, pa.Table), (table.combine_chunks().to_batches()[0], pa.RecordBatch),
                      (table.to_batches(max_chunksize=700), pa.Table)):
        train, test = splitter.split(src)
        for got, rows in ((train, want_train), (test, want_test)):
            assert isinstance(got, kind) and got.schema.equals(table.schema)
            assert got.to_pydict() == table.take(pa.array(rows)).to_pydict()
    # device tensors, custom column names, one extra column and one entry that is no tensor
    dev = {"u": torch.as_tensor(log["user_idx"]).to(DEV), "i": torch.as_tensor(log["item_idx"].astype(np.int32)).to(DEV),
           "t": torch.as_tensor(log["timestamp"].astype(np.int64)).to(DEV),
           "relevance": torch.as_tensor(log["relevance"]).to(DEV),
           "extra": torch.arange(len(frame), dtype=torch.float16, device=DEV), "name": "my log"}
    train, test = S.UserSplitter(user_col="u", item_col="i", date_col="t", **args).split(dev)
    for got, rows in ((train, want_train), (test, want_test)):
        assert set(got) == set(dev) and got["name"] == "my log"
        for k, v in dev.items():
            if torch.is_tensor(v):
                assert got[k].is_cuda and got[k].dtype == v.dtype
                assert torch.equal(got[k].cpu(), v.cpu()[torch.as_tensor(rows)])
    with pytest.raises(ValueError, match="no column"):
        splitter.split(dev)


def test_two_calls_return_identical_bytes():
    log = edge()
    dev = on_device(log, "int")
    for name, args in (("UserSplitter", dict(item_test_size=0.35, shuffle=True, user_test_size=0.3, seed=5,
                                             drop_cold_items=True, drop_cold_users=True)),
                       ("NewUsersSplitter", dict(test_size=0.25, drop_cold_items=True)),
                       ("DateSplitter", dict(test_start=0.2, drop_cold_items=True, drop_cold_users=True))):
        first = [t.cpu().numpy().tobytes() for t in CLASSES[name](**args).split_indices(dev)]
        again = [t.cpu().numpy().tobytes() for t in CLASSES[name](**args).split_indices(dev)]
        assert first == again


@pytest.mark.parametrize("n_folds", [2, 5])
def test_k_folds(n_folds):
    log = edge()
    frame = pd.DataFrame(log)
    want = R.fold_rows(log, n_folds, seed=11)
    tests = []
    for (train, test), (want_train, want_test) in zip(S.k_folds(frame, n_folds, seed=11), want):
        pd.testing.assert_frame_equal(train, frame.iloc[want_train].reset_index(drop=True))
        pd.testing.assert_frame_equal(test, frame.iloc[want_test].reset_index(drop=True))
        tests.append(want_test)
    assert len(tests) == n_folds
    assert np.array_equal(np.sort(np.concatenate(tests)), np.arange(len(frame)))        # the test parts partition the log
    per_user = np.stack([np.bincount(log["user_idx"][t], minlength=3000) for t in tests])
    assert (per_user.max(0) - per_user.min(0) <= 1).all()
    with pytest.raises(ValueError):
        next(S.k_folds(frame, 3, splitter="item"))


def test_empty_and_single_row_logs():
    cols = {"user_idx": np.zeros(0, np.int64), "item_idx": np.zeros(0, np.int64), "timestamp": np.zeros(0, np.int64),
            "relevance": np.zeros(0, np.float64)}
    one = {"user_idx": np.array([4]), "item_idx": np.array([2]), "timestamp": np.array([17]), "relevance": np.array([1.0])}
    splitters = [S.UserSplitter(), S.UserSplitter(item_test_size=0.5, shuffle=True), S.DateSplitter(0.5), S.DateSplitter(17),
                 S.RandomSplitter(0.5), S.NewUsersSplitter(0.5), S.ColdUserRandomSplitter(0.5)]
    for s in splitters:
        train, test = s.split(pd.DataFrame(cols))
        assert len(train) == 0 and len(test) == 0 and list(train.columns) == list(cols)
        train, test = s.split_indices(on_device(cols))
        assert train.numel() == 0 and test.numel() == 0 and train.dtype == torch.int64
        name = type(s).__name__
        args = {k: v for k, v in s._init_args.items() if k not in ("user_col", "item_col", "date_col")}
        train, test = check(name, args, one, on_device(one))
        assert len(train) + len(test) == 1
    assert [len(t) for _, t in S.k_folds(pd.DataFrame(one), 3)] in ([1, 0, 0], [0, 1, 0])       # rank 1 -> fold 1 % 3
    assert all(len(a) == 0 and len(b) == 0 for a, b in S.k_folds(pd.DataFrame(cols), 2))
    torch.cuda.synchronize()
    # ids are range-checked before any kernel indexes with them
    bad = dict(one, user_idx=np.array([-1]))
    with pytest.raises(ValueError, match="non-negative"):
        S.UserSplitter().split_indices(on_device(bad))
    with pytest.raises(ValueError, match="non-negative"):
        S.DateSplitter(0.5, drop_cold_items=True).split_indices(on_device(dict(one, item_idx=np.array([-5]))))


def test_split_fit_evaluate_end_to_end():
    from oracle import cql_oracle as O
    from replay_cql_amd.cql import CQL
    u, i, t, r = O.synth_log(120, 300, seed=4, mean_len=14, max_len=40)
    log = pd.DataFrame({"user_idx": u.astype(np.int32), "item_idx": i.astype(np.int32),
                        "timestamp": np.asarray(t).astype("datetime64[s]").astype("datetime64[us]"),
                        "relevance": np.asarray(r, dtype=np.float64)})
    train, test = S.UserSplitter(item_test_size=2, drop_cold_items=True, drop_cold_users=True).split(log)
    assert len(test) > 0 and len(train) + len(test) <= len(log)
    assert set(test.item_idx) <= set(train.item_idx) and set(test.user_idx) <= set(train.user_idx)
    model = CQL(embedding_dim=64, window=8, batch_size=64, n_steps=8, seed=3, device=DEV)
    model.fit_arrow(pa.Table.from_pandas(train, preserve_index=False))
    got = model.evaluate(train, test, ks=[5, 10])
    assert set(got) >= {"NDCG", "HitRate", "Precision", "Recall", "MAP", "MRR"}
    for metric, by_k in got.items():
        for k, v in by_k.items():
            assert np.isfinite(v) and 0.0 <= v <= 1.0, (metric, k, v)
