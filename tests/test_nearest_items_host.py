"""get_nearest_items on the host side (no GPU): the wrapper semantics of replay/models/base_rec.py:851-936 on a toy
`PandasRecommender`, the reference's own scenario (tests/models/test_all_models.py:211-236), the new C ABI entry points
(argument validation, workspace size) and the Spark adapter's routing through the stand-ins of test_spark_adapter.py."""
import numpy as np
import pandas as pd
import pytest

import knn_reference as R
from replay_cql_amd import _native as N
from replay_cql_amd import build as B
from replay_cql_amd.recommender_api import PandasRecommender
from replay_cql_amd.spark_adapter import build_adapter
from test_spark_adapter import REC_SCHEMA, FakeDF, FakeRecommender, FakeState


class Table(PandasRecommender):
    """item-to-item model over a small table of item vectors: `_get_nearest_items` returns EVERY admissible pair, as
    ItemVectorModel does (base_rec.py:968-1030); the wrapper under test picks the k best"""
    can_predict_item_to_item = True

    def __init__(self, vectors):
        self.vectors = np.asarray(vectors, dtype=np.float64)

    def _fit(self, log, user_features=None, item_features=None):
        pass

    def _predict(self, log, k, users, items, user_features=None, item_features=None, filter_seen_items=True):
        raise AssertionError("not used")

    def _get_nearest_items(self, items, metric=None, candidates=None):
        fit = self.fit_items["item_idx"].to_numpy()
        q = items["item_idx"][items["item_idx"].isin(fit)].to_numpy()
        c = fit if candidates is None else candidates["item_idx"][candidates["item_idx"].isin(fit)].to_numpy()
        val, ok = R.pair_values(self.vectors, q, c, metric)
        rows = [(q[a], c[b], val[a, b]) for a in range(len(q)) for b in range(len(c)) if ok[a, b]]
        return pd.DataFrame(rows, columns=["item_idx_one", "item_idx_two", metric])


def _log(items):
    n = len(items)
    return pd.DataFrame({"user_idx": np.arange(n) % 3, "item_idx": items, "timestamp": pd.to_datetime(np.arange(n), unit="s"),
                         "relevance": 1.0})


VEC = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 2.0], [1.0, 1.0], [2.0, 0.0], [0.0, 0.0]])


@pytest.fixture()
def toy():
    m = Table(VEC)
    m.fit(_log([0, 1, 2, 3, 4, 5]))
    return m


def test_wrapper_top_k_tie_rule_and_columns(toy):
    out = toy.get_nearest_items([0], 3, "dot_product")
    assert list(out.columns) == ["item_idx", "neighbour_item_idx", "dot_product"]
    assert out["item_idx"].dtype == np.int32 and out["neighbour_item_idx"].dtype == np.int32
    assert out["dot_product"].dtype == np.float64
    # dots of item 0 = (1,0): item 4 -> 2; items 1 and 3 -> 1 (tie: the LARGER id first); 2 and 5 -> 0
    assert out["neighbour_item_idx"].tolist() == [4, 3, 1] and out["dot_product"].tolist() == [2.0, 1.0, 1.0]
    assert toy.get_nearest_items([0], 5, "dot_product")["neighbour_item_idx"].tolist() == [4, 3, 1, 5, 2]
    # the query item is never its own neighbour, an equal vector under another id is
    cos = toy.get_nearest_items([0], 1, "cosine_similarity")
    assert list(cos.columns)[2] == "cosine_similarity" and cos["neighbour_item_idx"].tolist() == [4]
    assert toy.get_nearest_items([0], 2, "cosine_similarity")["neighbour_item_idx"].tolist() == [4, 1]
    euc = toy.get_nearest_items([0], 2, "euclidean_distance_sim")
    assert euc["neighbour_item_idx"].tolist() == [1, 5] and euc["euclidean_distance_sim"].tolist() == [1.0, 0.5]


def test_wrapper_k_candidates_and_ids(toy):
    assert len(toy.get_nearest_items([2], 50, "dot_product")) == 5                 # k above the number of candidates
    out = toy.get_nearest_items([0, 0, 2, 0], 2, "dot_product")                      # query ids are de-duplicated
    assert out.groupby("item_idx").size().to_dict() == {0: 2, 2: 2}
    out = toy.get_nearest_items(pd.DataFrame({"item_idx": [0]}), 5, "dot_product", candidates=[3, 1, 9, 0])
    assert out["neighbour_item_idx"].tolist() == [3, 1]                              # 9: not seen at fit; 0: the query
    assert len(toy.get_nearest_items([9], 3, "dot_product")) == 0                   # unknown query item: no rows
    with pytest.raises(ValueError, match="metric is required"):
        toy.get_nearest_items([0], 2, None)
    with pytest.raises(NotImplementedError, match="valid metrics"):
        toy.get_nearest_items([0], 2, "manhattan")


def test_reference_scenario():
    """tests/models/test_all_models.py:211-236 of the reference: fit without item 3, items = [0, 1]"""
    vec = np.random.default_rng(0).normal(size=(4, 8))
    m = Table(vec)
    m.fit(_log([0, 1, 2, 0, 1, 2]))
    for metric in R.METRICS:
        res = m.get_nearest_items([0, 1], 2, metric)
        assert len(res) == 4 and set(res["item_idx"]) == {0, 1}
        assert len(m.get_nearest_items([0, 1], 1, metric)) == 2
        res = m.get_nearest_items([0, 1], 4, metric, candidates=[0, 3])
        assert len(res) == 1
        assert res["item_idx"].tolist() == [1] and res["neighbour_item_idx"].tolist() == [0]


def test_model_without_the_capability_still_refuses():
    class Plain(Table):
        can_predict_item_to_item = False
    m = Plain(VEC)
    m.fit(_log([0, 1, 2]))
    with pytest.raises(NotImplementedError, match="item-to-item"):
        m.get_nearest_items([0], 2, "dot_product")


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def test_abi_workspace_and_validation_without_gpu(lib):
    import ctypes as C
    assert N.ITEM_KNN_MAX_K >= 512
    # two floats per (query, group of 32 candidates) + the gathered query block
    assert lib.cqlrec_item_knn_ws_bytes(1000, 100000, 128, 10) >= 2 * 3125 * 1000 * 4 + 1000 * 128 * 2
    a = lib.cqlrec_item_knn_ws_bytes(16384, 1000000, 256, 10)
    assert 0 < a < (1 << 30)                                           # more than 4096 groups: the groups grow instead
    assert lib.cqlrec_item_knn_ws_bytes(0, 100, 128, 10) == 0 and lib.cqlrec_item_knn_ws_bytes(10, 100, 100, 10) == 0
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def knn(E=p, nrm=p, n_rows=100, d=64, q=p, nq=4, cand=None, nc=100, metric=N.SIM_DOT, k=5, ws=p, wsb=1 << 40):
        return lib.cqlrec_item_knn(E, nrm, n_rows, d, q, nq, cand, nc, metric, k, ws, wsb, p, p, p, None)
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(knn(E=None))
    with pytest.raises(N.CqlrecError, match="unsupported"):
        N.check(knn(d=100))
    with pytest.raises(N.CqlrecError, match="metric"):
        N.check(knn(metric=3))
    with pytest.raises(N.CqlrecError, match=r"out of range \(1\.\.512\)"):
        N.check(knn(k=513))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(knn(k=0))
    with pytest.raises(N.CqlrecError, match="n_cand must equal n_rows"):
        N.check(knn(nc=50))
    with pytest.raises(N.CqlrecError, match="n_cand"):
        N.check(knn(cand=p, nc=101))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(knn(wsb=16))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_item_norms(None, 10, 64, p, None))
    with pytest.raises(N.CqlrecError, match="unsupported"):
        N.check(lib.cqlrec_item_norms(p, 10, 96, p, None))


def test_torch_operator_is_listed():
    from replay_cql_amd import torch_ops
    assert "item_knn" in torch_ops.OPS


# ------------------------------------------------------------------------------------------------ Spark adapter
class ItemRecommender(FakeRecommender):
    """what BaseRecommender adds around the hook for item-to-item models (base_rec.py:851-887, :542-558)"""
    can_predict_item_to_item = False

    def _get_ids(self, data, column):
        if isinstance(data, FakeDF):
            return data.select(column).distinct()
        return FakeDF(pd.DataFrame({column: pd.unique(pd.Series(list(data)))}))

    def get_nearest_items(self, items, k, metric="cosine_similarity", candidates=None):
        if metric is None:
            raise ValueError("Distance metric is required to get nearest items")
        if self.can_predict_item_to_item:
            return self._get_nearest_items_wrap(items=items, k=k, metric=metric, candidates=candidates)
        raise ValueError("Use models with attribute 'can_predict_item_to_item' set to True to get nearest items")


def test_spark_adapter_advertises_and_routes_to_the_arrow_call(monkeypatch):
    import pyarrow as pa
    from replay_cql_amd import arrow_io as A
    cls = build_adapter(ItemRecommender, FakeState, REC_SCHEMA)
    assert cls.can_predict_item_to_item is True
    m = cls(embedding_dim=64)
    calls = []

    def fake_arrow(items, k, metric="cosine_similarity", candidates=None):
        calls.append((np.asarray(items).tolist(), k, metric, None if candidates is None else np.asarray(candidates).tolist()))
        return pa.RecordBatch.from_arrays([pa.array([1, 1], pa.int32()), pa.array([7, 2], pa.int32()),
                                           pa.array([0.5, 0.25], pa.float64())], schema=A.neighbours_schema(metric))
    monkeypatch.setattr(m._impl, "nearest_items_arrow", fake_arrow)
    out = m.get_nearest_items([1, 1, 4], 2, "dot_product", candidates=FakeDF(pd.DataFrame({"item_idx": [7, 2, 7]})))
    assert calls == [([1, 4], 2, "dot_product", [7, 2])]
    assert isinstance(out, FakeDF) and out.columns == ["item_idx", "neighbour_item_idx", "dot_product"]
    assert out.toPandas()["neighbour_item_idx"].tolist() == [7, 2]
    with pytest.raises(ValueError):
        m.get_nearest_items([1], 2, None)
    # the full similarity frame is refused beyond what can be materialised, with a pointer to the real entry
    m._impl.fit_items = pd.DataFrame({"item_idx": np.arange(5000)})
    with pytest.raises(ValueError, match="get_nearest_items"):
        m._get_nearest_items(FakeDF(pd.DataFrame({"item_idx": [1]})), "dot_product", None)
