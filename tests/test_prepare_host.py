"""replay_cql_amd.filters and replay_cql_amd.indexer without a GPU: the modules import, the functions carry the
reference's signatures and defaults, every argument and column check raises its ValueError before a GPU is asked for, and
the host-only side of the f6 entry points (workspace queries, argument validation before any launch) behaves."""
import inspect
import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

import replay_cql_amd
from replay_cql_amd import _native as N
from replay_cql_amd import build as B
from replay_cql_amd import filters as F
from replay_cql_amd import indexer as I

ROOT = Path(__file__).resolve().parents[1]
E = inspect.Parameter.empty


def frame(**extra):
    cols = {"user_idx": np.array([0, 1, 1], dtype=np.int64), "item_idx": np.array([2, 0, 1], dtype=np.int32),
            "timestamp": np.array([3, 4, 5], dtype=np.int64), "relevance": np.array([1.0, 2.0, 3.0])}
    cols.update(extra)
    return pd.DataFrame(cols)


def cpu_tensors(**extra):
    cols = {"user_idx": torch.tensor([0, 1, 1]), "item_idx": torch.tensor([2, 0, 1]), "timestamp": torch.tensor([3, 4, 5]),
            "relevance": torch.tensor([1.0, 2.0, 3.0])}
    cols.update(extra)
    return cols


def test_package_exports_the_filters_and_the_indexer():
    for name in F.__all__:
        assert getattr(replay_cql_amd, name) is getattr(F, name) and name in replay_cql_amd.__all__
    assert replay_cql_amd.Indexer is I.Indexer and "Indexer" in replay_cql_amd.__all__
    assert len(F.__all__) == 6


def test_signatures_and_defaults_are_the_references():
    def params(fn):
        return [(p.name, p.default, p.kind == p.KEYWORD_ONLY) for p in inspect.signature(fn).parameters.values()]

    tail = [("return_rows", False, True)]
    assert params(F.filter_by_min_count) == [("data_frame", E, False), ("num_entries", E, False),
                                             ("group_by", "user_idx", False)] + tail
    assert params(F.filter_out_low_ratings) == [("data_frame", E, False), ("value", E, False),
                                                ("rating_column", "relevance", False)] + tail
    assert params(F.take_num_user_interactions) == [("log", E, False), ("num_interactions", 10, False),
                                                    ("first", True, False), ("date_col", "timestamp", False),
                                                    ("user_col", "user_idx", False), ("item_col", "item_idx", False)] + tail
    assert params(F.take_num_days_of_user_hist) == [("log", E, False), ("days", 10, False), ("first", True, False),
                                                    ("date_col", "timestamp", False), ("user_col", "user_idx", False)] + tail
    assert params(F.take_time_period) == [("log", E, False), ("start_date", None, False), ("end_date", None, False),
                                          ("date_column", "timestamp", False)] + tail
    assert params(F.take_num_days_of_global_hist) == [("log", E, False), ("duration_days", E, False),
                                                      ("first", True, False), ("date_column", "timestamp", False)] + tail
    assert [(p.name, p.default) for p in list(inspect.signature(I.Indexer.__init__).parameters.values())[1:]] == [
        ("user_col", "user_id"), ("item_col", "item_id")]
    for method, names in (("fit", ["users", "items"]), ("transform", ["df"]), ("inverse_transform", ["df"])):
        assert list(inspect.signature(getattr(I.Indexer, method)).parameters)[1:] == names


def test_indexer_init_args():
    assert I.Indexer()._init_args == {"user_col": "user_id", "item_col": "item_id"}
    ix = I.Indexer("u", item_col="i")
    assert ix._init_args == {"user_col": "u", "item_col": "i"}
    assert I.Indexer(**ix._init_args)._init_args == ix._init_args
    assert ix.user_labels is None and ix.item_labels is None
    with pytest.raises(ValueError, match="not fitted"):
        ix.transform(pd.DataFrame({"u": [1]}))


@pytest.mark.parametrize("log", [frame(), cpu_tensors(), pa.Table.from_pandas(frame())], ids=["pandas", "tensors", "arrow"])
@pytest.mark.parametrize("days", [1.0, 2.5, True, "3", None])
def test_non_integral_days_raise(log, days):
    with pytest.raises(ValueError, match="integer number of days"):
        F.take_num_days_of_user_hist(log, days)
    with pytest.raises(ValueError, match="integer number of days"):
        F.take_num_days_of_global_hist(log, days, first=False)


@pytest.mark.parametrize("kind", ["pandas", "arrow", "batches"])
def test_column_checks_come_before_the_gpu_is_asked_for(kind):
    def given(df):
        table = pa.Table.from_pandas(df, preserve_index=False)
        return {"pandas": df, "arrow": table, "batches": iter(table.to_batches(max_chunksize=2))}[kind]

    with pytest.raises(ValueError, match="integer column"):                       # a float group column
        F.filter_by_min_count(given(frame(user_idx=np.array([0.0, 1.0, 1.0]))), 2)
    with pytest.raises(ValueError, match="integer column"):                       # a string user column
        F.take_num_user_interactions(given(frame(user_idx=["a", "b", "b"])), 1)
    with pytest.raises(ValueError, match="integer column"):
        F.take_num_user_interactions(given(frame(item_idx=np.array([0.5, 1.0, 1.0]))), 1)
    with pytest.raises(ValueError, match="integer column"):
        F.take_num_days_of_user_hist(given(frame(user_idx=["a", "b", "b"])), 1)
    with pytest.raises(ValueError, match="no column"):
        F.filter_by_min_count(given(frame()), 2, group_by="shop")
    with pytest.raises(ValueError, match="no column"):
        F.filter_out_low_ratings(given(frame()), 2, rating_column="stars")
    with pytest.raises(ValueError, match="no column"):
        F.take_num_user_interactions(given(frame()), 2, date_col="when")
    with pytest.raises(ValueError, match="no column"):
        F.take_time_period(given(frame()), date_column="when")
    with pytest.raises(ValueError, match="no column"):
        F.take_num_days_of_global_hist(given(frame()), 1, date_column="when")
    with pytest.raises(ValueError, match="numeric"):
        F.filter_out_low_ratings(given(frame(relevance=["a", "b", "c"])), 2)
    with pytest.raises(ValueError, match="datetime, integer or float"):
        F.take_time_period(given(frame(timestamp=["a", "b", "c"])))
    # the Indexer: integer ids only, and the message says what to do instead
    with pytest.raises(ValueError, match="factorize"):
        I.Indexer("user_idx", "item_idx").fit(given(frame(user_idx=["a", "b", "b"])), given(frame()))
    with pytest.raises(ValueError, match="factorize"):
        I.Indexer("user_idx", "item_idx").fit(given(frame()), given(frame(item_idx=np.array([0.5, 1.0, 1.0]))))
    with pytest.raises(ValueError, match="no column"):
        I.Indexer().fit(given(frame()), given(frame()))


def test_column_checks_on_a_dict_of_tensors():
    with pytest.raises(ValueError, match="integer column"):
        F.filter_by_min_count(cpu_tensors(user_idx=torch.tensor([0.0, 1.0, 1.0])), 2)
    with pytest.raises(ValueError, match="no column"):
        F.take_num_days_of_user_hist(cpu_tensors(), 1, user_col="who")
    with pytest.raises(ValueError, match="factorize"):
        I.Indexer("user_idx", "item_idx").fit(cpu_tensors(user_idx=torch.tensor([0.0, 1.0, 1.0])), cpu_tensors())


@pytest.mark.parametrize("bad", ["yesterday", "2020-13-45", "01/02/2020", 1.5, object()])
def test_a_bound_that_is_no_date_raises(bad):
    with pytest.raises(ValueError):
        F.take_time_period(frame(), start_date=bad)
    with pytest.raises(ValueError):
        F.take_time_period(cpu_tensors(), end_date=bad)


def test_the_forms_of_a_bound():
    from datetime import datetime, timezone, timedelta
    from replay_cql_amd.splitters import _instant_ns
    ns = 1577887200 * 10 ** 9                                                     # 2020-01-01 14:00:00 UTC
    assert _instant_ns("2020-01-01 14:00:00") == _instant_ns(datetime(2020, 1, 1, 14)) == _instant_ns(1577887200) == ns
    assert _instant_ns(datetime(2020, 1, 1, 16, tzinfo=timezone(timedelta(hours=2)))) == ns
    assert _instant_ns("2020-01-01") == 1577836800 * 10 ** 9


def test_filters_and_indexer_refuse_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    calls = [lambda x: F.filter_by_min_count(x, 2), lambda x: F.filter_out_low_ratings(x, 2.0),
             lambda x: F.take_num_user_interactions(x, 1), lambda x: F.take_num_days_of_user_hist(x, 1),
             lambda x: F.take_time_period(x, "2020-01-01"), lambda x: F.take_num_days_of_global_hist(x, 1),
             lambda x: I.Indexer("user_idx", "item_idx").fit(x, x)]
    for call in calls:
        for log in (frame(), cpu_tensors(), pa.Table.from_pandas(frame())):
            with pytest.raises(N.CqlrecError, match="no CPU path"):
                call(log)


def test_importing_the_package_and_the_modules_does_not_initialise_the_gpu():
    code = ("import sys, replay_cql_amd, replay_cql_amd.filters, replay_cql_amd.indexer\n"
            "from replay_cql_amd import Indexer, filter_by_min_count\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n"
            "assert Indexer('a', 'b')._init_args == {'user_col': 'a', 'item_col': 'b'}\n"
            "assert not torch.cuda.is_initialized()\n"
            "print('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]
    code = "import sys, replay_cql_amd\nassert 'torch' not in sys.modules and 'replay_cql_amd.filters' not in sys.modules\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_prepare_entry_points_validate_on_the_host():
    B.build(verbose=False)
    lib = N.load()
    assert lib.cqlrec_prepare_rank_ws_bytes(1000, 10) > 1000 * 24
    assert lib.cqlrec_prepare_rank_ws_bytes(2000, 10) > lib.cqlrec_prepare_rank_ws_bytes(1000, 10)
    assert lib.cqlrec_prepare_rank_ws_bytes(-1, 10) == 0
    assert lib.cqlrec_prepare_compact_ws_bytes(1000) > 8000
    assert lib.cqlrec_prepare_distinct_ws_bytes(1000) > 8000
    assert lib.cqlrec_prepare_sort_labels_ws_bytes(1000) > 4000
    big = 1 << 31
    buf = (N.C.c_int64 * 64)()
    p = N.C.addressof(buf)
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_rank(None, None, None, big, 10, 0, None, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="n_key2"):
        N.check(lib.cqlrec_prepare_rank(p, p, p, 10, 10, 0, p, 0, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_rank(None, None, None, 10, 10, 0, None, 0, None, p, None))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(lib.cqlrec_prepare_rank(p, p, None, 10, 10, 0, p, 64, p, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_count(None, -1, 10, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_count(None, 10, 10, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_minmax(None, None, 10, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="one group"):
        N.check(lib.cqlrec_prepare_minmax(None, p, 10, 5, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_minmax(p, None, 10, 5, p, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_keep(0, None, None, None, None, None, None, big, 1, 1, 0, 0, 0, 0, 0.0, None, None))
    with pytest.raises(N.CqlrecError, match="unknown rule"):
        N.check(lib.cqlrec_prepare_keep(6, None, None, None, None, None, None, 10, 1, 1, 0, 0, 0, 0, 0.0, None, None))
    for rule in range(6):                                  # every rule reads at least one array
        with pytest.raises(N.CqlrecError, match="NULL"):
            N.check(lib.cqlrec_prepare_keep(rule, None, None, None, None, None, None, 10, 1, 1, 0, 0, 0, 0, 0.0, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_keep(3, p, p, None, None, None, p, 10, 1, 1, 0, 0, 0, 0, 0.0, None, None))
    assert lib.cqlrec_prepare_keep(5, None, None, None, None, None, None, 0, 0, 1, 0, 0, 0, 0, 0.0, None, None) == 0
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_compact(None, big, None, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_compact(None, 10, None, 0, None, p, None))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(lib.cqlrec_prepare_compact(p, 10, p, 64, p, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_distinct(None, -5, None, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(lib.cqlrec_prepare_distinct(p, 10, p, 64, p, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_sort_labels(None, big, None, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_sort_labels(None, 10, None, 0, None, None, None))
    assert lib.cqlrec_prepare_sort_labels(None, 0, None, 0, None, None, None) == 0
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_lookup(None, big, None, None, 1, None, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_lookup(None, 10, None, None, 1, None, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_prepare_gather(None, 10, None, -1, None, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_prepare_gather(None, 10, None, 1, None, None, None))
