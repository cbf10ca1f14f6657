"""replay_cql_amd.neighbour without a GPU: the classes carry the reference's arguments, flags and error texts, the
package exports them, the library exports every f8 symbol, and the host-only side of the f8 entry points (workspace
queries, argument validation before any launch, the "no dense buffer" condition) behaves."""
import inspect
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import replay_cql_amd
from replay_cql_amd import _native as N
from replay_cql_amd import build as B
from replay_cql_amd import _similarity as SIM
from replay_cql_amd import neighbour as NB

ROOT = Path(__file__).resolve().parents[1]
F8 = ["cqlrec_neighbour_weights", "cqlrec_neighbour_norms", "cqlrec_neighbour_count_ws_bytes", "cqlrec_neighbour_count",
      "cqlrec_neighbour_topk_ws_bytes", "cqlrec_neighbour_topk", "cqlrec_neighbour_pair_scores"]


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def frame():
    return pd.DataFrame({"user_idx": np.array([0, 1, 2, 2], dtype=np.int64), "item_idx": np.array([0, 1, 0, 1], dtype=np.int64),
                         "relevance": np.ones(4)})


def test_package_exports_the_models():
    assert NB.__all__ == ["NeighbourRec", "ItemKNN"]
    for name in NB.__all__:
        assert getattr(replay_cql_amd, name) is getattr(NB, name) and name in replay_cql_amd.__all__
    assert issubclass(NB.ItemKNN, NB.NeighbourRec)
    from replay_cql_amd.recommender_api import PandasRecommender
    assert issubclass(NB.NeighbourRec, PandasRecommender)


def test_constructor_arguments_and_errors():
    params = list(inspect.signature(NB.ItemKNN.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("num_neighbours", 10), ("use_relevance", False), ("shrink", 0.0),
                                                     ("weighting", None), ("max_tuples", 1 << 27)]
    assert params[-1].kind is inspect.Parameter.KEYWORD_ONLY
    m = NB.ItemKNN(7, True, 2.5, "bm25", max_tuples=64)
    assert m._init_args == {"shrink": 2.5, "use_relevance": True, "num_neighbours": 7, "weighting": "bm25"}
    assert m.max_tuples == 64 and str(m) == "ItemKNN"
    assert (NB.ItemKNN.bm25_k1, NB.ItemKNN.bm25_b) == (1.2, 0.75)
    assert NB.ItemKNN._search_space == {"num_neighbours": {"type": "int", "args": [1, 100]},
                                        "shrink": {"type": "int", "args": [0, 100]},
                                        "weighting": {"type": "categorical", "args": [None, "tf_idf", "bm25"]}}
    for bad in (" ", "tfidf", "BM25", 0):
        with pytest.raises(ValueError, match=r"^weighting must be one of \[None, 'tf_idf', 'bm25'\]$"):
            NB.ItemKNN(weighting=bad)


def test_flags_and_the_similarity_metric():
    m = NB.ItemKNN()
    assert m.can_predict_item_to_item and m.can_predict_cold_users and not m.can_predict_cold_items
    assert not m.can_change_metric and m.item_to_item_metrics == ["similarity"] and m.similarity_metric == "similarity"
    with pytest.raises(ValueError, match="^This class does not support changing similarity metrics$"):
        m.similarity_metric = "similarity"

    class Changeable(NB.ItemKNN):
        can_change_metric = True
        item_to_item_metrics = ["similarity", "lift"]
    c = Changeable()
    with pytest.raises(ValueError, match=r"^Select one of the valid metrics for predict: \['similarity', 'lift'\]$"):
        c.similarity_metric = "confidence"
    c.similarity_metric = "lift"
    assert c.similarity_metric == "lift" and NB.ItemKNN().similarity_metric == "similarity"


def test_unfitted_and_logless_calls_raise():
    m = NB.ItemKNN()
    with pytest.raises(RuntimeError, match="not fitted"):
        m.similarity_device
    with pytest.raises(RuntimeError, match="not fitted"):
        m.predict(frame(), 1)
    with pytest.raises(RuntimeError, match="not fitted"):
        m.recommend(frame(), 1)
    m._clear_cache()                                        # nothing to drop yet
    m._sim = SIM.Padded(torch.zeros((2, 1), dtype=torch.int32), {"similarity": torch.zeros((2, 1), dtype=torch.float64)},
                        torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="^log is not provided, but it is required for prediction$"):
        m.recommend(None, 1)
    with pytest.raises(ValueError, match="^log is not provided, but it is required for prediction$"):
        m._predict_pairs(frame()[["user_idx", "item_idx"]], None)
    assert list(m.similarity.columns) == ["item_idx_one", "item_idx_two", "similarity"] and len(m.similarity) == 0
    assert m._dataframes["similarity"] is m.similarity


def test_the_models_refuse_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        NB.ItemKNN().fit(frame())
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        NB.ItemKNN().fit({"user_idx": torch.tensor([0, 1]), "item_idx": torch.tensor([0, 1])})


def test_importing_the_module_does_not_initialise_the_gpu():
    code = ("import replay_cql_amd.neighbour, torch\nfrom replay_cql_amd import ItemKNN\nItemKNN(3, weighting='tf_idf')\n"
            "assert not torch.cuda.is_initialized()\nprint('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]
    code = "import sys, replay_cql_amd\nassert 'replay_cql_amd.neighbour' not in sys.modules\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_every_f8_symbol_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cqlrec.h").read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cqlrec_neighbour_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(F8)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (cqlrec_neighbour_[a-z0-9_]+)", nm))
    assert exported == set(F8)
    assert all(name in N.SIGNATURES for name in F8)
    assert lib.cqlrec_abi_version() == 2 == N.ABI_VERSION
    assert "neighbour.hip" in B.SOURCES and "-ffp-contract=off" in B.EXTRA["neighbour.hip"]
    assert (N.NEIGHBOUR_FIT, N.NEIGHBOUR_PREDICT, N.NEIGHBOUR_MAX_K) == (0, 1, 1024)


def test_workspace_queries_and_the_no_dense_buffer_condition(lib):
    ws, cnt = lib.cqlrec_neighbour_topk_ws_bytes, lib.cqlrec_neighbour_count_ws_bytes
    assert cnt(1000) > 1001 * 8 and cnt(0) > 0 and cnt(-1) == 0 and cnt(1 << 31) == 0
    good = (1000, 1000, 4096, 10, 10)
    assert ws(*good) > 4096 * 56
    for bad in ((-1, 1000, 4096, 10, 10), (1 << 31, 1000, 4096, 10, 10), (1000, -1, 4096, 10, 10),
                (1000, 1 << 31, 4096, 10, 10), (1000, 1000, 0, 10, 10), (1000, 1000, 4096, -1, 10),
                (1000, 1000, 4096, 10, 0), (1000, 1000, 4096, 10, 1025), (1000, 1000, 1 << 31, 10, 10),
                (1000, 1000, 4096, 1 << 31, 10)):
        assert ws(*bad) == 0, bad
    assert ws(1000, 1000, 4096, 10, 1) > 0 and ws(1000, 1000, 4096, 10, 1024) > 0
    # the workspace holds max(max_tuples, largest row) tuples, and grows by no more than 88 bytes (+ alignment) per tuple
    assert ws(1000, 1000, 64, 5000, 10) == ws(1000, 1000, 5000, 5000, 10) > ws(1000, 1000, 64, 10, 10)
    assert ws(1000, 1000, 2 << 20, 10, 10) - ws(1000, 1000, 1 << 20, 10, 10) <= 96 << 20
    # no buffer of n_q x n_cols or n_cols x n_cols elements: doubling the columns at N = 10^6 adds at most 64 N bytes
    n = 10 ** 6
    for k in (10, 1024):
        assert 0 <= ws(n, 2 * n, 1 << 20, 1 << 16, k) - ws(n, n, 1 << 20, 1 << 16, k) <= 64 * n
    # O(max_tuples + rows): the query rows cost their offsets, nothing like n_q x n_cols
    assert ws(2 * n, n, 1 << 20, 1 << 16, 10) - ws(n, n, 1 << 20, 1 << 16, 10) <= 16 * n


def test_f8_entry_points_validate_on_the_host(lib):
    big = 1 << 31
    buf = (N.C.c_int64 * 64)()
    p = N.C.addressof(buf)
    # weights
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_weights(p, p, p, p, p, big, 10, 0, 1.2, 0.75, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_weights(p, p, p, p, p, 10, -1, 0, 1.2, 0.75, p, None))
    with pytest.raises(N.CqlrecError, match="unknown weighting"):
        N.check(lib.cqlrec_neighbour_weights(p, p, p, p, p, 10, 10, 3, 1.2, 0.75, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_neighbour_weights(p, p, p, p, p, 10, 10, 0, 1.2, 0.75, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_neighbour_weights(p, p, p, None, p, 10, 10, 1, 1.2, 0.75, p, None))
    with pytest.raises(N.CqlrecError, match="n_items > 0"):
        N.check(lib.cqlrec_neighbour_weights(p, p, p, p, p, 10, 0, 2, 1.2, 0.75, p, None))
    assert lib.cqlrec_neighbour_weights(None, None, None, None, None, 0, 0, 0, 1.2, 0.75, None, None) == 0
    # norms
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_norms(p, p, p, big, 10, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_norms(p, p, p, 10, 0, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_neighbour_norms(p, p, p, 10, 10, None, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_neighbour_norms(None, p, p, 10, 10, p, None))
    # the count pass
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_count(p, p, big, 10, p, 10, p, 1 << 30, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_count(p, p, 10, -1, p, 10, p, 1 << 30, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_neighbour_count(p, p, 10, 10, p, 10, p, 1 << 30, p, p, None, None))
    # the engine
    def topk(mode=0, n_q=4, nnz=8, n_mid=4, n_cols=4, prefix=(0, 1, 2, 3, 4), max_tuples=64, largest=1, k=2, norm=p, ws=p,
             ws_bytes=1 << 30, out=p, seen_off=None, seen_col=None, l=p):
        host = (N.C.c_int64 * max(1, len(prefix)))(*prefix)
        return lib.cqlrec_neighbour_topk(mode, l, l, l, n_q, nnz, p, p, p, n_mid, n_cols, p, host if prefix else None,
                                         max_tuples, largest, k, norm, norm, 0.0, None, seen_off, seen_col, ws, ws_bytes, out,
                                         out, out, None)
    with pytest.raises(N.CqlrecError, match="unknown mode"):
        N.check(topk(mode=2))
    for bad in (dict(n_q=-1), dict(n_q=big), dict(nnz=big), dict(n_mid=-1), dict(n_cols=big)):
        with pytest.raises(N.CqlrecError, match="out of range"):
            N.check(topk(**bad))
    for k in (0, -1, 1025):
        with pytest.raises(N.CqlrecError, match=r"k=-?\d+ out of range"):
            N.check(topk(k=k))
    for bad in (dict(max_tuples=0), dict(largest=-1), dict(max_tuples=big), dict(largest=big)):
        with pytest.raises(N.CqlrecError, match="max_tuples=.* out of range"):
            N.check(topk(**bad))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(topk(out=None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(topk(prefix=()))
    with pytest.raises(N.CqlrecError, match="does not start at 0"):
        N.check(topk(prefix=(1, 1, 2, 3, 4)))
    with pytest.raises(N.CqlrecError, match="row 2 expands to 5 tuples, largest_row is 1"):
        N.check(topk(prefix=(0, 1, 2, 7, 8)))
    with pytest.raises(N.CqlrecError, match="row 1 expands to -1 tuples"):
        N.check(topk(prefix=(0, 1, 0, 1, 2)))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(topk(l=None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(topk(ws=None))
    with pytest.raises(N.CqlrecError, match="FIT needs the norms"):
        N.check(topk(norm=None))
    with pytest.raises(N.CqlrecError, match="seen lists"):
        N.check(topk(mode=1, seen_off=p))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(topk(ws_bytes=64))
    assert topk(n_q=0, prefix=(), out=None, l=None, ws=None) == 0
    # pair scores
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_pair_scores(p, p, big, p, p, 10, p, p, p, 10, p, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_neighbour_pair_scores(p, p, 10, p, p, -1, p, p, p, 10, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_neighbour_pair_scores(p, None, 10, p, p, 10, p, p, p, 10, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_neighbour_pair_scores(p, p, 10, None, p, 10, p, p, p, 10, p, p, None))
    assert lib.cqlrec_neighbour_pair_scores(None, None, 0, None, None, 0, None, None, None, 0, None, None, None) == 0
