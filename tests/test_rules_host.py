"""replay_cql_amd.association_rules without a GPU: the class carries the reference's arguments, flags and error texts, the
package exports it lazily, the library exports every f10 symbol, and the host-only side of the f10 entry points
(workspace query, argument validation before any launch) behaves."""
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
from replay_cql_amd import _similarity as SIM
from replay_cql_amd import association_rules as AR
from replay_cql_amd import build as B
from replay_cql_amd import neighbour as NB

ROOT = Path(__file__).resolve().parents[1]
F10 = ["cqlrec_rules_distinct", "cqlrec_rules_topk_ws_bytes", "cqlrec_rules_topk"]
METRICS = ["lift", "confidence", "confidence_gain"]


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def frame():
    return pd.DataFrame({"user_idx": np.array([0, 1, 2, 2], dtype=np.int64), "item_idx": np.array([0, 1, 0, 1], dtype=np.int64),
                         "relevance": np.ones(4)})


def test_package_exports_the_model():
    assert AR.__all__ == ["AssociationRulesItemRec"]
    assert replay_cql_amd.AssociationRulesItemRec is AR.AssociationRulesItemRec
    assert "AssociationRulesItemRec" in replay_cql_amd.__all__
    assert issubclass(AR.AssociationRulesItemRec, NB.NeighbourRec)


def test_constructor_arguments_init_args_and_str():
    params = list(inspect.signature(AR.AssociationRulesItemRec.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [
        ("session_col", None), ("min_item_count", 5), ("min_pair_count", 5), ("num_neighbours", 1000),
        ("use_relevance", False), ("similarity_metric", "confidence"), ("max_tuples", NB.DEFAULT_MAX_TUPLES)]
    assert params[-1].kind is inspect.Parameter.KEYWORD_ONLY
    m = AR.AssociationRulesItemRec()
    assert m._init_args == {"session_col": "user_idx", "min_item_count": 5, "min_pair_count": 5, "num_neighbours": 1000,
                            "use_relevance": False, "similarity_metric": "confidence"}
    assert str(m) == "AssociationRulesItemRec" and m.max_tuples == NB.DEFAULT_MAX_TUPLES
    m = AR.AssociationRulesItemRec("session", 2, 3, None, True, "lift", max_tuples=64)
    assert m._init_args == {"session_col": "session", "min_item_count": 2, "min_pair_count": 3, "num_neighbours": None,
                            "use_relevance": True, "similarity_metric": "lift"}
    assert m.max_tuples == 64
    assert AR.AssociationRulesItemRec._search_space == {
        "min_item_count": {"type": "int", "args": [3, 10]},
        "min_pair_count": {"type": "int", "args": [3, 10]},
        "num_neighbours": {"type": "int", "args": [300, 2000]},
        "use_relevance": {"type": "categorical", "args": [True, False]},
        "similarity_metric": {"type": "categorical", "args": ["confidence", "lift"]},
    }


def test_flags_and_the_two_error_messages():
    m = AR.AssociationRulesItemRec()
    assert m.can_predict_item_to_item and m.can_change_metric and m.can_predict_cold_users
    assert m.item_to_item_metrics == METRICS and m.similarity_metric == "confidence"
    for metric in METRICS:
        m.similarity_metric = metric
        assert m.similarity_metric == metric and m._init_args["similarity_metric"] == metric
    with pytest.raises(ValueError, match=r"^Select one of the valid metrics for predict: \['lift', 'confidence', 'confidence_gain'\]$"):
        m.similarity_metric = "similarity"
    with pytest.raises(ValueError, match=r"^Select one of the valid metrics for predict: "):
        AR.AssociationRulesItemRec(similarity_metric="cosine")
    with pytest.raises(ValueError, match=r"^Select one of the valid distance metrics: \['lift', 'confidence', 'confidence_gain'\]$"):
        m.get_nearest_items([1], 2, metric="similarity")
    assert inspect.signature(m.get_nearest_items).parameters["metric"].default == "lift"
    assert NB.ItemKNN().similarity_metric == "similarity"                     # the base class keeps its single plane


def test_the_metric_picks_the_plane_and_the_csr_cache_follows():
    """host tensors stand in for a fitted table: the helpers only index them"""
    m = AR.AssociationRulesItemRec()
    with pytest.raises(RuntimeError, match="not fitted"):
        m.similarity_device
    ids = torch.tensor([[1, -1], [0, 2], [1, -1]], dtype=torch.int32)
    planes = [torch.tensor([[x, 0.0], [x + 1, x + 2], [x + 3, 0.0]], dtype=torch.float64) for x in (10.0, 20.0, 30.0)]
    m._sim = SIM.Padded(ids, dict(zip(("confidence", "lift", "confidence_gain"), planes)), torch.tensor([1, 2, 1], dtype=torch.int32))
    assert len(m.similarity_device) == 5
    assert list(m.similarity.columns) == ["item_idx_one", "item_idx_two", "confidence", "lift", "confidence_gain"]
    assert m.similarity["item_idx_one"].tolist() == [0, 1, 1, 2] and m.similarity["item_idx_two"].tolist() == [1, 0, 2, 1]
    assert m.similarity["lift"].tolist() == [20.0, 21.0, 22.0, 23.0]
    assert m.get_similarity is m.similarity and m._dataframes["similarity"] is m.similarity
    for metric, base in (("confidence", 10.0), ("lift", 20.0), ("confidence_gain", 30.0), ("confidence", 10.0)):
        m.similarity_metric = metric
        assert m._sim.plane(m.similarity_metric) is planes[("confidence", "lift", "confidence_gain").index(metric)]
        (off, col, val), (_, col_sorted, val_sorted) = m._csr(4)
        assert off.tolist() == [0, 1, 3, 4, 4] and col.tolist() == [1, 0, 2, 1]
        assert val.tolist() == [base, base + 1, base + 2, base + 3] == val_sorted.tolist()
        assert m._csr(4)[0][2] is val                                          # cached until the metric or the size changes
    out = m.get_nearest_items([1], 1, "confidence_gain")
    assert out.to_dict("list") == {"item_idx": [1], "neighbour_item_idx": [2], "confidence_gain": [32.0]}
    out = m.get_nearest_items([1, 0], 5, candidates=[0, 1])
    assert list(out.columns) == ["item_idx", "neighbour_item_idx", "lift"] and sorted(out["lift"]) == [20.0, 21.0]
    with pytest.raises(ValueError, match="^log is not provided, but it is required for prediction$"):
        m.recommend(None, 1)
    m._clear_cache()
    assert "_csr_cache" not in m.__dict__ and "_similarity_frame" not in m.__dict__


def test_the_model_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        AR.AssociationRulesItemRec().fit(frame())
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        AR.AssociationRulesItemRec().fit({"user_idx": torch.tensor([0, 1]), "item_idx": torch.tensor([0, 1])})
    m = AR.AssociationRulesItemRec()
    m._sim = SIM.Padded(torch.zeros((2, 1), dtype=torch.int32),
                        {name: torch.zeros((2, 1), dtype=torch.float64) for name in ("confidence", "lift", "confidence_gain")}, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        m.recommend(frame(), 1)
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        m._predict_pairs(frame()[["user_idx", "item_idx"]], frame())


def test_importing_the_package_neither_imports_the_module_nor_initialises_the_gpu():
    code = "import sys, replay_cql_amd\nassert 'replay_cql_amd.association_rules' not in sys.modules\nassert 'torch' not in sys.modules\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    code = ("import torch\nfrom replay_cql_amd import AssociationRulesItemRec\nAssociationRulesItemRec('session', similarity_metric='lift')\n"
            "assert not torch.cuda.is_initialized()\nprint('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]


def test_every_f10_symbol_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cqlrec.h").read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cqlrec_rules_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(F10)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r" T (cqlrec_rules_[a-z0-9_]+)", nm)) == set(F10)
    assert all(name in N.SIGNATURES and hasattr(lib, name) for name in F10)
    assert lib.cqlrec_abi_version() == 2 == N.ABI_VERSION
    assert "f10" in (ROOT / "include" / "cqlrec.h").read_text()


def test_the_workspace_query_is_host_only_and_rejects_what_is_out_of_range(lib):
    ws, nb = lib.cqlrec_rules_topk_ws_bytes, lib.cqlrec_neighbour_topk_ws_bytes
    assert ws(1000, 4096, 10, 10) == nb(1000, 1000, 4096, 10, 10) > 4096 * 56
    for bad in ((-1, 4096, 10, 10), (1 << 31, 4096, 10, 10), (1000, 0, 10, 10), (1000, 4096, -1, 10), (1000, 4096, 10, 0),
                (1000, 4096, 10, 1025), (1000, 1 << 31, 10, 10), (1000, 4096, 1 << 31, 10)):
        assert ws(*bad) == 0, bad
    assert ws(1000, 4096, 10, 1) > 0 and ws(1000, 4096, 10, 1024) > 0
    assert ws(1000, 64, 5000, 10) == ws(1000, 5000, 5000, 10) > ws(1000, 64, 10, 10)
    # bounded by max_tuples, never n_items x n_items: doubling the items at N = 10^6 adds their offsets only
    n = 10 ** 6
    assert 0 <= ws(2 * n, 1 << 20, 1 << 16, 1024) - ws(n, 1 << 20, 1 << 16, 1024) <= 16 * n


def test_f10_entry_points_validate_on_the_host(lib):
    big = 1 << 31
    buf = (N.C.c_int64 * 64)()
    p = N.C.addressof(buf)
    # the mark
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_rules_distinct(p, p, p, p, big, p, None))
    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_rules_distinct(p, p, p, p, -1, p, None))
    for args in ((None, p, p, p), (p, None, p, p), (p, p, p, None)):
        with pytest.raises(N.CqlrecError, match="NULL"):
            N.check(lib.cqlrec_rules_distinct(*args, 10, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_rules_distinct(p, p, None, p, 10, None, None))
    assert lib.cqlrec_rules_distinct(None, None, None, None, 0, None, None) == 0

    # the engine
    def topk(n_items=4, nnz=8, n_sessions=4, prefix=(0, 1, 2, 3, 4), max_tuples=64, largest=1, k=2, num_sessions=4,
             min_pair_count=1, ws=p, ws_bytes=1 << 30, out=p, item_rel=p, l=p, l_off=p):
        host = (N.C.c_int64 * max(1, len(prefix)))(*prefix)
        return lib.cqlrec_rules_topk(l_off, l, l, n_items, nnz, p, p, p, n_sessions, p, host if prefix else None, max_tuples,
                                     largest, k, num_sessions, min_pair_count, ws, ws_bytes, out, out, out, out, out,
                                     item_rel, None)
    for bad in (dict(n_items=-1), dict(n_items=big), dict(nnz=big), dict(nnz=-1), dict(n_sessions=-1), dict(n_sessions=big)):
        with pytest.raises(N.CqlrecError, match="out of range"):
            N.check(topk(**bad))
    for k in (0, -1, 1025):
        with pytest.raises(N.CqlrecError, match=r"k=-?\d+ out of range \(1\.\.1024\)"):
            N.check(topk(k=k))
    for bad in (dict(max_tuples=0), dict(largest=-1), dict(max_tuples=big), dict(largest=big)):
        with pytest.raises(N.CqlrecError, match="max_tuples=.* out of range"):
            N.check(topk(**bad))
    for bad in (dict(num_sessions=-1), dict(num_sessions=5)):
        with pytest.raises(N.CqlrecError, match="num_sessions=-?\\d+ out of range"):
            N.check(topk(**bad))
    for bad in (dict(out=None), dict(prefix=()), dict(item_rel=None), dict(l_off=None), dict(l=None), dict(ws=None)):
        with pytest.raises(N.CqlrecError, match="NULL"):
            N.check(topk(**bad))
    with pytest.raises(N.CqlrecError, match="does not start at 0"):
        N.check(topk(prefix=(1, 1, 2, 3, 4)))
    with pytest.raises(N.CqlrecError, match="rules_topk: row 2 expands to 5 tuples, largest_row is 1"):
        N.check(topk(prefix=(0, 1, 2, 7, 8)))
    with pytest.raises(N.CqlrecError, match="row 1 expands to -1 tuples"):
        N.check(topk(prefix=(0, 1, 0, 1, 2)))
    with pytest.raises(N.CqlrecError, match="workspace too small"):
        N.check(topk(ws_bytes=64))
    assert topk(n_items=0, prefix=(), out=None, item_rel=None, l=None, l_off=None, ws=None) == 0
