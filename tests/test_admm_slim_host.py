"""replay_cql_amd.admm_slim without a GPU: the class carries the reference's arguments, attributes and error text, the
package exports it lazily, the library exports every f11 symbol, and the host-only side of the f11 entry points
(workspace queries, argument validation before any launch) behaves."""
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
from replay_cql_amd import build as B
from replay_cql_amd import neighbour as NB

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "admm_slim_known_answers.json").read_text())
F11 = ["cqlrec_admm_compact", "cqlrec_admm_iteration", "cqlrec_admm_iteration_ws_bytes", "cqlrec_dense_gemm_f64",
       "cqlrec_dense_gram", "cqlrec_dense_gram_ws_bytes", "cqlrec_dense_spd_inverse", "cqlrec_dense_spd_inverse_ws_bytes"]


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def frame():
    return pd.DataFrame({"user_idx": np.array([0, 1, 2, 2], dtype=np.int64), "item_idx": np.array([0, 1, 0, 1], dtype=np.int64),
                         "relevance": np.ones(4)})


def test_package_exports_the_model():
    assert AS.__all__ == ["ADMMSLIM"]
    assert replay_cql_amd.ADMMSLIM is AS.ADMMSLIM and "ADMMSLIM" in replay_cql_amd.__all__
    assert issubclass(AS.ADMMSLIM, NB.NeighbourRec)


def test_constructor_arguments_attributes_and_errors():
    params = list(inspect.signature(AS.ADMMSLIM.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("lambda_1", 5), ("lambda_2", 5000), ("seed", None)]
    m = AS.ADMMSLIM()
    assert m._init_args == {"lambda_1": 5, "lambda_2": 5000, "seed": None} and m.rho == 5000 and str(m) == "ADMMSLIM"
    assert AS.ADMMSLIM(0.5, 4, 42)._init_args == {"lambda_1": 0.5, "lambda_2": 4, "seed": 42}
    assert (m.threshold, m.multiplicator, m.eps_abs, m.eps_rel, m.max_iteration) == (5, 2, 1e-3, 1e-3, 100)
    assert AS.ADMMSLIM._search_space == {"lambda_1": {"type": "loguniform", "args": [1e-9, 50]},
                                         "lambda_2": {"type": "loguniform", "args": [1e-9, 5000]}}
    for bad in ((-1, 5), (5, 0), (5, -2), (-0.1, 0)):
        with pytest.raises(ValueError, match="^Invalid regularization parameters$"):
            AS.ADMMSLIM(*bad)
    AS.ADMMSLIM(0, 1e-9)
    assert m.can_predict_item_to_item and m.can_predict_cold_users and not m.can_change_metric
    assert m.similarity_metric == "similarity"
    with pytest.raises(ValueError, match="does not support changing similarity metrics"):
        m.similarity_metric = "lift"


def test_the_csr_table_serves_the_base_class():
    """host tensors stand in for a fitted table: the helpers only index them"""
    m = AS.ADMMSLIM()
    with pytest.raises(RuntimeError, match="not fitted"):
        m.similarity_device
    with pytest.raises(RuntimeError, match="not fitted"):
        m.recommend(frame(), 1)
    m._sim = SIM.Csr(torch.tensor([0, 1, 3, 3], dtype=torch.int64), torch.tensor([2, 0, 1], dtype=torch.int32),
                     torch.tensor([0.5, -0.25, 1.5], dtype=torch.float64))
    assert m._n_rows() == 3 and len(m.similarity_device) == 3
    sim = m.similarity
    assert sim.to_dict("list") == {"item_idx_one": [0, 1, 1], "item_idx_two": [2, 0, 1], "similarity": [0.5, -0.25, 1.5]}
    assert [str(t) for t in sim.dtypes] == ["int32", "int32", "float64"] and m._dataframes["similarity"] is sim
    (off, col, val), by_col = m._csr(5)
    assert off.tolist() == [0, 1, 3, 3, 3, 3] and col is m._sim[1] and val is m._sim[2] and by_col[1] is col
    assert m._csr(5)[0][0] is off and m._csr(3)[0][0] is m._sim[0]
    out = m.get_nearest_items([1], 1)
    assert out.to_dict("list") == {"item_idx": [1], "neighbour_item_idx": [1], "similarity": [1.5]}
    with pytest.raises(ValueError, match="^log is not provided, but it is required for prediction$"):
        m.recommend(None, 1)
    m._clear_cache()
    assert "_csr_cache" not in m.__dict__ and "_similarity_frame" not in m.__dict__
    knn = NB.ItemKNN()                                   # the padded table of the other models counts its rows as before
    knn._sim = SIM.Padded(torch.zeros((4, 2), dtype=torch.int32), {"similarity": torch.zeros((4, 2), dtype=torch.float64)},
                          torch.zeros(4, dtype=torch.int32))
    assert knn._n_rows() == 4


def test_the_model_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        AS.ADMMSLIM().fit(frame())
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        AS.ADMMSLIM().fit({"user_idx": torch.tensor([0, 1]), "item_idx": torch.tensor([0, 1])})
    m = AS.ADMMSLIM()
    m._sim = SIM.Csr(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64))
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        m.recommend(frame(), 1)
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        m._predict_pairs(frame()[["user_idx", "item_idx"]], frame())


def test_importing_the_package_neither_imports_the_module_nor_initialises_the_gpu():
    code = "import sys, replay_cql_amd\nassert 'replay_cql_amd.admm_slim' not in sys.modules\nassert 'torch' not in sys.modules\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    code = ("import torch\nfrom replay_cql_amd import ADMMSLIM\nADMMSLIM(1, 2, seed=3)\n"
            "assert not torch.cuda.is_initialized()\nprint('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]


def test_every_f11_symbol_is_declared_exported_and_bound(lib):
    text = (ROOT / "include" / "cqlrec.h").read_text()
    assert "f11" in text and "CQLREC_DENSE_GRAM_PIECE 1024" in text and "CQLREC_DENSE_BLOCK 64" in text
    assert (N.DENSE_GRAM_PIECE, N.DENSE_BLOCK) == (1024, 64)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cqlrec_(?:dense|admm)_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(F11)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r" T (cqlrec_(?:dense|admm)_[a-z0-9_]+)", nm)) == set(F11)
    assert all(name in N.SIGNATURES and hasattr(lib, name) for name in F11)
    assert "dense.hip" in B.SOURCES and "-ffp-contract=off" in B.EXTRA["dense.hip"]


def test_the_workspace_queries_are_host_only_and_known(lib):
    for name, table in GOLDEN["ws_bytes"].items():
        fn = getattr(lib, f"cqlrec_{name}_ws_bytes")
        for sizes, want in table.items():
            assert fn(*[int(x) for x in sizes.split(",")]) == want, (name, sizes)
    inv, it, gram = lib.cqlrec_dense_spd_inverse_ws_bytes, lib.cqlrec_admm_iteration_ws_bytes, lib.cqlrec_dense_gram_ws_bytes
    for n in (1, 64, 65, 130, 8192, 40000):
        assert 2 * 8 * n * n <= inv(n) <= int(2.3 * 8 * n * n) + 4096          # the working copy, L^-1, a quarter for a product
        assert 8 * n * n <= it(n) <= 8 * n * n + 8 * n + 40 * (n // 128 + 1) ** 2 + 1024   # rho C - Gamma, v and the tile sums
    # five resident matrices of an iteration, 40 n^2 bytes: the largest n the entry points take fits a card of 288 GB
    assert 4 * 8 * 65536 ** 2 + it(65536) < 200 * 10 ** 9
    for bad in (0, -1, (1 << 16) + 1):
        assert inv(bad) == 0 and it(bad) == 0 and gram(bad, 0) == 0
    assert gram(10, -1) == 0 and gram(130, 3) - gram(130, 0) >= 3 * 130 * 8


def test_f11_entry_points_validate_on_the_host(lib):
    buf = (N.C.c_double * 64)()
    p = N.C.addressof(buf)

    def gemm(A=p, lda=4, ta=0, B=p, ldb=4, tb=0, E=None, lde=0, alpha=1.0, beta=0.0, m=4, n=4, k=4, D=p, ldd=4):
        return lib.cqlrec_dense_gemm_f64(A, lda, ta, B, ldb, tb, E, lde, alpha, beta, m, n, k, D, ldd, None)
    for bad in (dict(m=0), dict(n=-1), dict(k=0), dict(k=1 << 31), dict(m=(1 << 22) + 1), dict(ta=2), dict(tb=-1)):
        with pytest.raises(N.CqlrecError, match="out of range"):
            N.check(gemm(**bad))
    for bad in (dict(A=None), dict(B=None), dict(D=None), dict(beta=1.0)):
        with pytest.raises(N.CqlrecError, match="NULL"):
            N.check(gemm(**bad))
    for bad in (dict(lda=3), dict(ldb=3), dict(ldd=3), dict(E=p, lde=3, beta=2.0), dict(ta=1, m=8, k=4, lda=4), dict(tb=1, n=2, k=8, ldb=4)):
        with pytest.raises(N.CqlrecError, match="leading dimension"):
            N.check(gemm(**bad))

    with pytest.raises(N.CqlrecError, match="out of range"):
        N.check(lib.cqlrec_dense_gram(p, p, p, p, p, p, 0, 4, 0, p, 1 << 20, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_dense_gram(None, p, p, p, p, p, 4, 4, 0, p, 1 << 20, p, None))
    with pytest.raises(N.CqlrecError, match="workspace holds 8 bytes"):
        N.check(lib.cqlrec_dense_gram(p, p, p, p, p, p, 4, 4, 0, p, 8, p, None))

    with pytest.raises(N.CqlrecError, match=r"n=0 out of range \(1\.\.65536\)"):
        N.check(lib.cqlrec_dense_spd_inverse(p, 4, 0, 0.0, p, 1 << 20, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_dense_spd_inverse(p, 4, 4, 0.0, p, 1 << 20, p, None, None))
    with pytest.raises(N.CqlrecError, match="lda=3 is shorter"):
        N.check(lib.cqlrec_dense_spd_inverse(p, 3, 4, 0.0, p, 1 << 20, p, p, None))
    with pytest.raises(N.CqlrecError, match="workspace holds 64 bytes"):
        N.check(lib.cqlrec_dense_spd_inverse(p, 4, 4, 0.0, p, 64, p, p, None))

    def iteration(n=4, rho=1.0, lambda_1=0.5, ws=p, ws_bytes=1 << 20, C=p, sums=p):
        return lib.cqlrec_admm_iteration(p, p, C, p, n, rho, lambda_1, ws, ws_bytes, sums, None)
    for bad, text in ((dict(n=0), "n=0 out of range"), (dict(rho=0.0), "rho=0"), (dict(rho=float("nan")), "rho=nan"),
                      (dict(lambda_1=-1.0), "lambda_1=-1"), (dict(C=None), "NULL"), (dict(sums=None), "NULL"), (dict(ws=None), "NULL"),
                      (dict(ws_bytes=8), "workspace holds 8 bytes")):
        with pytest.raises(N.CqlrecError, match=text):
            N.check(iteration(**bad))

    for bad, text in ((dict(n=0), "out of range"), (dict(n_rows=3), "out of range"), (dict(C=None), "NULL"), (dict(off=None), "NULL"),
                      (dict(col=p), "NULL")):
        a = dict(C=p, n=4, n_rows=4, off=p, col=None, val=None)
        a.update(bad)
        with pytest.raises(N.CqlrecError, match=text):
            N.check(lib.cqlrec_admm_compact(a["C"], a["n"], a["n_rows"], a["off"], a["col"], a["val"], None))
