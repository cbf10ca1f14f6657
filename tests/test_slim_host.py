"""replay_cql_amd.slim without a GPU: the class carries the reference's arguments, attributes and error text, the package
exports it lazily, the library exports every f12 symbol, and the host-only side of the f12 entry points (the workspace
query, argument validation before any launch) behaves."""
import inspect
import json
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
from replay_cql_amd import admm_slim as AS
from replay_cql_amd import association_rules as AR
from replay_cql_amd import build as B
from replay_cql_amd import neighbour as NB
from replay_cql_amd import slim as SL

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "slim_known_answers.json").read_text())
F12 = ["cqlrec_slim_fit", "cqlrec_slim_fit_ws_bytes"]


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def frame():
    return pd.DataFrame({"user_idx": np.array([0, 1, 2, 2], dtype=np.int64), "item_idx": np.array([0, 1, 0, 1], dtype=np.int64),
                         "relevance": np.ones(4)})


def test_package_exports_the_model():
    assert SL.__all__ == ["SLIM"]
    assert replay_cql_amd.SLIM is SL.SLIM and "SLIM" in replay_cql_amd.__all__
    for model in (NB.ItemKNN, AR.AssociationRulesItemRec, AS.ADMMSLIM, SL.SLIM):     # one implementation: NeighbourRec's
        assert model.__mro__[1] is NB.NeighbourRec
        for name in ("similarity", "similarity_device", "_csr", "_n_rows", "_dataframes"):
            assert name not in vars(model) and getattr(model, name) is getattr(NB.NeighbourRec, name), (model, name)


def test_constructor_arguments_attributes_and_errors():
    params = list(inspect.signature(SL.SLIM.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("beta", 0.01), ("lambda_", 0.01), ("seed", None)]
    m = SL.SLIM()
    assert m._init_args == {"beta": 0.01, "lambda_": 0.01, "seed": None} and str(m) == "SLIM"
    assert SL.SLIM(0.5, 4, 42)._init_args == {"beta": 0.5, "lambda_": 4, "seed": 42}
    assert (m.tol, m.max_iter) == (1e-4, 5000) and (SL.SLIM.tol, SL.SLIM.max_iter) == (1e-4, 5000)
    assert SL.SLIM._search_space == {"beta": {"type": "loguniform", "args": [1e-6, 5]},
                                     "lambda_": {"type": "loguniform", "args": [1e-6, 2]}}
    for bad in ((-1, 5), (5, 0), (5, -2), (-0.1, 0)):
        with pytest.raises(ValueError, match="^Invalid regularization parameters$"):
            SL.SLIM(*bad)
    SL.SLIM(0, 1e-9)
    assert m.can_predict_item_to_item and m.can_predict_cold_users and not m.can_change_metric
    assert m.similarity_metric == "similarity"
    with pytest.raises(ValueError, match="does not support changing similarity metrics"):
        m.similarity_metric = "lift"
    assert "deterministic" in SL.SLIM.__init__.__doc__ and "unused" in SL.SLIM.__init__.__doc__
    assert "tol * lambda_" in SL.__doc__


def test_the_csr_table_serves_the_base_class():
    """host tensors stand in for a fitted table: the helpers only index them"""
    m = SL.SLIM()
    with pytest.raises(RuntimeError, match="not fitted"):
        m.similarity_device
    with pytest.raises(RuntimeError, match="not fitted"):
        m.recommend(frame(), 1)
    m._sim = SIM.Csr(torch.tensor([0, 1, 3, 3], dtype=torch.int64), torch.tensor([2, 0, 1], dtype=torch.int32),
                     torch.tensor([0.5, 0.25, 1.5], dtype=torch.float64))
    assert m._n_rows() == 3 and len(m.similarity_device) == 3
    sim = m.similarity
    assert sim.to_dict("list") == {"item_idx_one": [0, 1, 1], "item_idx_two": [2, 0, 1], "similarity": [0.5, 0.25, 1.5]}
    assert [str(t) for t in sim.dtypes] == ["int32", "int32", "float64"] and m._dataframes["similarity"] is sim
    (off, col, val), by_col = m._csr(5)
    assert off.tolist() == [0, 1, 3, 3, 3, 3] and col is m._sim[1] and val is m._sim[2] and by_col[1] is col
    out = m.get_nearest_items([1], 1)
    assert out.to_dict("list") == {"item_idx": [1], "neighbour_item_idx": [1], "similarity": [1.5]}
    with pytest.raises(ValueError, match="^log is not provided, but it is required for prediction$"):
        m.recommend(None, 1)
    m._clear_cache()
    assert "_csr_cache" not in m.__dict__ and "_similarity_frame" not in m.__dict__


def test_the_model_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        SL.SLIM().fit(frame())
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        SL.SLIM().fit({"user_idx": torch.tensor([0, 1]), "item_idx": torch.tensor([0, 1])})
    m = SL.SLIM()
    m._sim = SIM.Csr(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64))
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        m.recommend(frame(), 1)
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        m._predict_pairs(frame()[["user_idx", "item_idx"]], frame())


def test_importing_the_package_neither_imports_the_module_nor_initialises_the_gpu():
    code = "import sys, replay_cql_amd\nassert 'replay_cql_amd.slim' not in sys.modules\nassert 'torch' not in sys.modules\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    code = ("import torch\nfrom replay_cql_amd import SLIM\nSLIM(1, 2, seed=3)\n"
            "assert not torch.cuda.is_initialized()\nprint('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]


def test_every_f12_symbol_is_declared_exported_and_bound(lib):
    text = (ROOT / "include" / "cqlrec.h").read_text()
    assert "f12" in text and "CQLREC_SLIM_MAX_ITEMS 16384" in text and "#define CQLREC_ABI_VERSION 2" in text
    assert N.SLIM_MAX_ITEMS == 16384 == GOLDEN["cap"] and N.ABI_VERSION == 2 == lib.cqlrec_abi_version()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cqlrec_slim_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(F12)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r" T (cqlrec_slim_[a-z0-9_]+)", nm)) == set(F12)
    assert all(name in N.SIGNATURES and hasattr(lib, name) for name in F12)
    assert "slim.hip" in B.SOURCES and B.EXTRA["slim.hip"] == ["-ffp-contract=off"]
    assert "cqlrec_slim_" not in (ROOT / "replay_cql_amd" / "csrc" / "torch_ops.cpp").read_text()    # no torch.ops twins


def test_the_workspace_query_is_host_only_and_known(lib):
    fn = lib.cqlrec_slim_fit_ws_bytes
    assert sorted(GOLDEN["ws_bytes"]) == sorted(str(n) for n in (1, 64, 1025, 16384, 16385))
    for n, want in GOLDEN["ws_bytes"].items():
        assert fn(int(n)) == want, n
    assert fn(16384) > 0 and fn(16385) == 0 and fn(0) == 0 and fn(-1) == 0
    for n in (1, 64, 1025, 16384):
        assert fn(n) >= 8 * n * 2 and fn(n) % 256 == 0
    assert fn(16384) < 1 << 27                                     # G itself is 2 GiB there: the workspace is small beside it


def test_slim_fit_validates_on_the_host(lib):
    buf = (N.C.c_double * 64)()
    p = N.C.addressof(buf)

    def fit(G=p, ldg=4, n=4, n_users=3, beta=0.01, lambda_=0.01, tol=1e-4, max_iter=10, col_begin=0, col_end=4, ws=p,
            ws_bytes=1 << 30, S=p, lds=4, sweeps=p, kkt=p, updates=p):
        return lib.cqlrec_slim_fit(G, ldg, n, n_users, beta, lambda_, tol, max_iter, col_begin, col_end, ws, ws_bytes, S, lds,
                                   sweeps, kkt, updates, None)
    for bad, text in ((dict(n=0), r"n=0 out of range \(1\.\.16384\)"), (dict(n=16385, ldg=16385, lds=16385, col_end=16385), "n=16385 out of range"),
                      (dict(n_users=0), "n_users=0 out of range"), (dict(beta=-1.0), "beta=-1 out of range"),
                      (dict(beta=float("nan")), "beta=nan"), (dict(lambda_=0.0), "lambda_=0 out of range"),
                      (dict(lambda_=-0.5), "lambda_=-0.5"), (dict(lambda_=float("inf")), "lambda_=inf"), (dict(tol=0.0), "tol=0 out of range"),
                      (dict(tol=float("nan")), "tol=nan"), (dict(max_iter=0), "max_iter=0 out of range"),
                      (dict(col_begin=-1), "columns -1..4 out of range"), (dict(col_begin=2, col_end=2), "columns 2..2 out of range"),
                      (dict(col_end=5), "columns 0..5 out of range"), (dict(col_begin=3, col_end=1), "columns 3..1"),
                      (dict(ldg=3), "leading dimension ldg=3"), (dict(lds=3), "lds=3 is shorter"),
                      (dict(G=None), "NULL"), (dict(S=None), "NULL"), (dict(sweeps=None), "NULL"), (dict(kkt=None), "NULL"),
                      (dict(updates=None), "NULL"), (dict(ws=None), "NULL"), (dict(ws_bytes=8), "workspace holds 8 bytes")):
        with pytest.raises(N.CqlrecError, match=text):
            N.check(fit(**bad))
