"""replay_cql_amd.history_based_fp without a GPU: the module imports, the classes carry the reference's signatures,
defaults and error texts, the column checks raise before a GPU is asked for, and the host-only side of the f7 entry
points (workspace queries, argument validation before any launch) behaves."""
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
from replay_cql_amd import history_based_fp as H

ROOT = Path(__file__).resolve().parents[1]
E = inspect.Parameter.empty


def frame(**extra):
    cols = {"user_idx": np.array([0, 1, 1], dtype=np.int64), "item_idx": np.array([2, 0, 1], dtype=np.int32),
            "timestamp": np.array([3, 4, 5], dtype=np.int64), "relevance": np.array([1.0, 2.0, 3.0])}
    cols.update(extra)
    return pd.DataFrame(cols)


def cpu_tensors():
    return {"user_idx": torch.tensor([0, 1, 1]), "item_idx": torch.tensor([2, 0, 1]), "timestamp": torch.tensor([3, 4, 5]),
            "relevance": torch.tensor([1.0, 2.0, 3.0])}


def params(fn):
    return [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]


def test_package_exports_the_processors():
    assert H.__all__ == ["EmptyFeatureProcessor", "LogStatFeaturesProcessor", "ConditionalPopularityProcessor",
                         "HistoryBasedFeaturesProcessor"]
    for name in H.__all__:
        assert getattr(replay_cql_amd, name) is getattr(H, name) and name in replay_cql_amd.__all__


def test_signatures_and_defaults_are_the_references():
    assert params(H.EmptyFeatureProcessor.fit) == [("log", E), ("features", None)]
    assert params(H.EmptyFeatureProcessor.transform) == [("log", E)]
    assert params(H.LogStatFeaturesProcessor.fit) == [("log", E), ("features", None)]
    assert params(H.LogStatFeaturesProcessor.transform) == [("log", E)]
    assert params(H.ConditionalPopularityProcessor.__init__) == [("cat_features_list", E)]
    assert params(H.ConditionalPopularityProcessor.fit) == [("log", E), ("features", E)]
    assert params(H.ConditionalPopularityProcessor.transform) == [("log", E)]
    assert params(H.HistoryBasedFeaturesProcessor.__init__) == [
        ("use_log_features", True), ("use_conditional_popularity", True), ("user_cat_features_list", None),
        ("item_cat_features_list", None)]
    assert params(H.HistoryBasedFeaturesProcessor.fit) == [("log", E), ("user_features", None), ("item_features", None)]
    assert params(H.HistoryBasedFeaturesProcessor.transform) == [("log", E)]
    for cls in (H.LogStatFeaturesProcessor, H.ConditionalPopularityProcessor, H.HistoryBasedFeaturesProcessor):
        assert params(cls.transform_block) == [("user_idx", E), ("item_idx", E), ("dtype", torch.float32)]
    assert issubclass(H.LogStatFeaturesProcessor, H.EmptyFeatureProcessor)
    assert issubclass(H.ConditionalPopularityProcessor, H.EmptyFeatureProcessor)
    assert H.LogStatFeaturesProcessor.calc_timestamp_based is False and H.LogStatFeaturesProcessor.calc_relevance_based is False


def test_which_processors_the_pipeline_builds():
    fp = H.HistoryBasedFeaturesProcessor()
    assert fp.fitted is False and type(fp.log_processor) is H.LogStatFeaturesProcessor
    assert type(fp.user_cond_pop_proc) is H.EmptyFeatureProcessor and type(fp.item_cond_pop_proc) is H.EmptyFeatureProcessor
    fp = H.HistoryBasedFeaturesProcessor(use_log_features=False, user_cat_features_list=["gender"],
                                         item_cat_features_list=["class"])
    assert type(fp.log_processor) is H.EmptyFeatureProcessor
    assert fp.user_cond_pop_proc.cat_features_list == ["gender"] and fp.item_cond_pop_proc.cat_features_list == ["class"]
    fp = H.HistoryBasedFeaturesProcessor(use_conditional_popularity=False, user_cat_features_list=["gender"])
    assert type(fp.user_cond_pop_proc) is H.EmptyFeatureProcessor
    # the deviation from the reference: the item list alone is enough
    fp = H.HistoryBasedFeaturesProcessor(item_cat_features_list=["class"])
    assert type(fp.item_cond_pop_proc) is H.ConditionalPopularityProcessor


def test_transform_before_fit_raises_the_references_error():
    for call in (lambda: H.HistoryBasedFeaturesProcessor().transform(frame()),
                 lambda: H.HistoryBasedFeaturesProcessor().transform_block(torch.tensor([0]), torch.tensor([0])),
                 lambda: H.LogStatFeaturesProcessor().transform(frame()),
                 lambda: H.ConditionalPopularityProcessor(["a"]).transform(frame())):
        with pytest.raises(AttributeError, match="^Call fit before running transform$"):
            call()
    assert H.EmptyFeatureProcessor().transform("anything") == "anything"
    assert H.EmptyFeatureProcessor().fit(frame(), None) is None
    assert H.LogStatFeaturesProcessor().user_log_features is None


@pytest.mark.parametrize("kind", ["pandas", "arrow", "batches"])
def test_column_checks_come_before_the_gpu_is_asked_for(kind):
    def given(df):
        table = pa.Table.from_pandas(df, preserve_index=False)
        return {"pandas": df, "arrow": table, "batches": iter(table.to_batches(max_chunksize=2))}[kind]

    with pytest.raises(ValueError, match="integer column"):
        H.LogStatFeaturesProcessor().fit(given(frame(user_idx=["a", "b", "b"])))
    with pytest.raises(ValueError, match="integer column"):
        H.LogStatFeaturesProcessor().fit(given(frame(item_idx=np.array([0.5, 1.0, 1.0]))))
    with pytest.raises(ValueError, match="no column"):
        H.LogStatFeaturesProcessor().fit(given(frame().drop(columns=["relevance"])))
    with pytest.raises(ValueError, match="numeric"):
        H.LogStatFeaturesProcessor().fit(given(frame(relevance=["a", "b", "c"])))
    features = pd.DataFrame({"user_idx": [0, 1], "gender": ["M", "F"]})
    with pytest.raises(ValueError) as err:
        H.ConditionalPopularityProcessor(["gender", "age"]).fit(given(frame()), features)
    assert str(err.value) == ("Columns {'age'} defined in `cat_features_list` are absent in features. "
                              "features columns are: ['user_idx', 'gender'].")
    with pytest.raises(ValueError, match="integer column"):
        H.ConditionalPopularityProcessor(["gender"]).fit(given(frame(item_idx=["a", "b", "b"])), features)
    with pytest.raises(ValueError, match="non-negative dense indices"):
        H.ConditionalPopularityProcessor(["gender"]).fit(given(frame()), features.assign(user_idx=[-1, 0]))


def test_the_processors_refuse_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    features = pd.DataFrame({"user_idx": [0, 1], "gender": ["M", "F"]})
    calls = [lambda x: H.LogStatFeaturesProcessor().fit(x), lambda x: H.ConditionalPopularityProcessor(["gender"]).fit(x, features),
             lambda x: H.HistoryBasedFeaturesProcessor().fit(x)]
    for call in calls:
        for log in (frame(), cpu_tensors(), pa.Table.from_pandas(frame())):
            with pytest.raises(N.CqlrecError, match="no CPU path"):
                call(log)
    fp = H.HistoryBasedFeaturesProcessor()
    fp.fitted = True
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        fp.transform_block(torch.tensor([0]), torch.tensor([0]))
    with pytest.raises(ValueError, match="float32 or float64"):
        fp.transform_block(torch.tensor([0]), torch.tensor([0]), torch.float16)


def test_importing_the_module_does_not_initialise_the_gpu():
    code = ("import sys, replay_cql_amd, replay_cql_amd.history_based_fp\n"
            "from replay_cql_amd import HistoryBasedFeaturesProcessor\n"
            "import torch\n"
            "fp = HistoryBasedFeaturesProcessor(user_cat_features_list=['a'])\n"
            "assert not torch.cuda.is_initialized() and not fp.fitted\n"
            "print('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]
    code = "import sys, replay_cql_amd\nassert 'replay_cql_amd.history_based_fp' not in sys.modules\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_features_entry_points_validate_on_the_host():
    B.build(verbose=False)
    lib = N.load()
    for query in (lib.cqlrec_features_segments_ws_bytes, lib.cqlrec_features_segment_stats_ws_bytes,
                  lib.cqlrec_features_segment_mean_ws_bytes):
        assert query(1000, 10) > 0 and query(200000, 10) > query(1000, 10) and query(1000, 100000) >= query(1000, 10)
        assert query(-1, 10) == 0 and query(10, -1) == 0
    assert lib.cqlrec_features_segments_ws_bytes(1000, 10) > 1000 * 24
    assert lib.cqlrec_features_segment_stats_ws_bytes(1 << 20, 10) >= ((1 << 20) // 1024 + 10) * 8 + 2 * 11 * 8
    assert lib.cqlrec_features_pair_counts_ws_bytes(1000) > 1000 * 20 and lib.cqlrec_features_pair_counts_ws_bytes(-1) == 0
    big = 1 << 31
    buf = (N.C.c_int64 * 64)()
    p = N.C.addressof(buf)
    # day
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_day(None, big, 86400, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_day(p, 10, 0, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_features_day(None, 10, 86400, p, None))
    assert lib.cqlrec_features_day(None, 0, 86400, None, None) == 0
    # segments
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_segments(None, None, big, 10, None, 0, None, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_segments(p, None, -1, 10, p, 0, p, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_segments(p, None, 10, 0, p, 0, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_features_segments(None, None, 10, 10, None, 0, None, p, None))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(lib.cqlrec_features_segments(p, None, 10, 10, p, 64, p, p, None))
    # segment statistics
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_segment_stats(None, None, None, big, 10, None, 0, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_segment_stats(p, p, p, 10, big, p, 0, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_features_segment_stats(None, None, None, 10, 10, None, 0, p, None))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(lib.cqlrec_features_segment_stats(p, p, p, 10, 10, p, 64, p, None))
    # segmented means
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_segment_mean(0, None, None, None, None, None, None, 1, 0.0, 0.0, -1, 10, None, 0, None, None))
    with pytest.raises(N.CqlrecError, match="unknown rule"):
        N.check(lib.cqlrec_features_segment_mean(3, p, p, p, p, p, p, 1, 0.0, 1.0, 10, 10, p, 0, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_features_segment_mean(0, None, None, None, None, None, None, 1, 0.0, 0.0, 10, 10, None, 0, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):                      # a stride of 0
        N.check(lib.cqlrec_features_segment_mean(0, p, p, None, p, p, None, 0, 0.0, 0.0, 10, 10, p, 1 << 30, p, None))
    with pytest.raises(N.CqlrecError, match="needs the value column"):
        N.check(lib.cqlrec_features_segment_mean(1, p, p, None, p, p, None, 1, 0.0, 0.0, 10, 10, p, 1 << 30, p, None))
    with pytest.raises(N.CqlrecError, match="min_std < max_std"):
        N.check(lib.cqlrec_features_segment_mean(2, p, p, p, p, p, p, 1, 1.0, 1.0, 10, 10, p, 1 << 30, p, None))
    with pytest.raises(N.CqlrecError, match="min_std < max_std"):       # NaN bounds
        N.check(lib.cqlrec_features_segment_mean(2, p, p, p, p, p, p, 1, float("nan"), 1.0, 10, 10, p, 1 << 30, p, None))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(lib.cqlrec_features_segment_mean(0, p, p, None, p, p, None, 1, 0.0, 0.0, 10, 10, p, 64, p, None))
    # distinct keys
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_segment_distinct(None, None, None, None, big, 10, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_features_segment_distinct(None, None, None, None, 10, 10, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_features_segment_distinct(p, p, p, p, 10, 10, None, None))
    # pair counts
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_pair_counts(None, None, None, None, big, 10, 3, None, 0, None, None, None, None, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_features_pair_counts(p, p, p, p, 10, 10, -1, p, 0, p, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_features_pair_counts(None, None, None, None, 10, 10, 3, None, 0, None, None, p, p, None))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(lib.cqlrec_features_pair_counts(p, p, p, p, 10, 10, 3, p, 64, p, p, p, p, None))
    # the block
    def block(n_pairs=10, n_users=5, fu=2, n_items=5, fi=2, colmap=(0, 0, 0), n_cols=1, pops=None, n_pop=0, dtype=0,
              user=p, tabs=p, out=p):
        cm = (N.C.c_int32 * len(colmap))(*colmap)
        return lib.cqlrec_features_block(user, user, n_pairs, tabs, tabs, n_users, fu, tabs, tabs, n_items, fi, cm, n_cols,
                                         pops, n_pop, dtype, out, None)
    for bad in (dict(n_pairs=big), dict(n_pairs=-1), dict(n_users=big), dict(n_cols=0), dict(n_cols=N.FEATURES_MAX_COLS + 1),
                dict(fu=-1), dict(n_pop=N.FEATURES_MAX_POP + 1)):
        with pytest.raises(N.CqlrecError, match="out of range"):
            N.check(block(**bad))
    with pytest.raises(N.CqlrecError, match="unknown dtype"):
        N.check(block(dtype=2))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(block(tabs=None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(block(user=None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(block(out=None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(block(colmap=(6, 0, 0), n_pop=1))
    for colmap in ((0, 2, 0), (1, -1, 0), (4, 0, 2), (5, 2, 0), (6, 0, 0), (7, 1, 0), (8, 0, 0), (-1, 0, 0)):
        with pytest.raises(N.CqlrecError, match="column 0"):
            N.check(block(colmap=colmap))
    pops = (N.FeaturesPop * 1)(N.FeaturesPop(None, None, None, None, None, 4, 5, 2, 3, 1, 0))
    with pytest.raises(N.CqlrecError, match="popularity table 0: NULL"):
        N.check(block(colmap=(6, 0, 0), pops=pops, n_pop=1))
    pops[0].m = -1
    with pytest.raises(N.CqlrecError, match="popularity table 0: sizes"):
        N.check(block(colmap=(6, 0, 0), pops=pops, n_pop=1))
    assert block(n_pairs=0, user=None, out=None) == 0
