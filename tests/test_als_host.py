"""replay_cql_amd.als without a GPU: the class carries the reference's arguments, the package exports it, the library
exports every f9 symbol, and the host-only side of the f9 entry points (workspace queries, argument validation before
any launch) behaves."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import als_reference as R
import replay_cql_amd
from replay_cql_amd import _native as N
from replay_cql_amd import als as ALS
from replay_cql_amd import build as B

ROOT = Path(__file__).resolve().parents[1]
F9 = ["cqlrec_als_gram_ws_bytes", "cqlrec_als_gram", "cqlrec_als_normal_equations_ws_bytes", "cqlrec_als_normal_equations",
      "cqlrec_als_half_step_ws_bytes", "cqlrec_als_half_step", "cqlrec_als_topk", "cqlrec_als_pair_scores"]


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def test_package_exports_the_model(lib):
    assert ALS.__all__ == ["ALSWrap"] and replay_cql_amd.ALSWrap is ALS.ALSWrap and "ALSWrap" in replay_cql_amd.__all__
    from replay_cql_amd.recommender_api import PandasRecommender
    assert issubclass(ALS.ALSWrap, PandasRecommender)
    assert all(name in N.SIGNATURES and hasattr(lib, name) for name in F9)
    assert "als.hip" in B.SOURCES and "-ffp-contract=off" in B.EXTRA["als.hip"]


def test_constants_match_the_header():
    text = (ROOT / "include" / "cqlrec.h").read_text()
    val = {k: int(v) for k, v in re.findall(r"#define CQLREC_ALS_([A-Z_]+) (\d+)", text)}
    assert val == {"PIECE": N.ALS_PIECE, "GRAM_BLOCK": N.ALS_GRAM_BLOCK, "MAX_RANK": N.ALS_MAX_RANK, "MAX_K": N.ALS_MAX_K,
                   "EXPLICIT": N.ALS_EXPLICIT, "IMPLICIT": N.ALS_IMPLICIT}
    assert (ALS.PIECE, ALS.MAX_RANK, ALS.MAX_K) == (N.ALS_PIECE, N.ALS_MAX_RANK, N.ALS_MAX_K) and R.PIECE == N.ALS_PIECE


def test_constructor_arguments_and_errors():
    params = list(inspect.signature(ALS.ALSWrap.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("rank", 10), ("implicit_prefs", True), ("seed", None), ("max_iter", 10),
                                                     ("reg_param", 0.1), ("alpha", 1.0)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[3:])
    m = ALS.ALSWrap(7, False, 42)
    assert m._init_args == {"rank": 7, "implicit_prefs": False, "seed": 42} and str(m) == "ALSWrap"
    assert ALS.ALSWrap()._init_args == {"rank": 10, "implicit_prefs": True, "seed": None}
    assert ALS.ALSWrap._search_space == {"rank": {"type": "loguniform_int", "args": [8, 256]}}
    assert not m.can_predict_cold_users and not m.can_predict_cold_items and not m.can_predict_item_to_item
    for bad in (0, 129, -3, 2.5, True):
        with pytest.raises(ValueError, match="rank must be an integer in 1..128"):
            ALS.ALSWrap(rank=bad)
    assert ALS.ALSWrap(rank=128).rank == 128 and ALS.ALSWrap(rank=1).rank == 1
    with pytest.raises(ValueError, match="non-negative"):
        ALS.ALSWrap(reg_param=-1.0)
    with pytest.raises(NotImplementedError):
        m.get_nearest_items([1], 3)
    for call in (lambda: m.factors_device("user"), lambda: m.recommend(None, 3), lambda: m._get_item_vectors()):
        with pytest.raises(RuntimeError, match="ALSWrap model is not fitted"):
            call()


def test_initial_factors_are_a_function_of_the_seed():
    m = ALS.ALSWrap()
    a, b, c = (m._init_factors(40, 10, s, device="cpu") for s in (7, 7, 8))
    assert a.dtype == torch.float32 and a.shape == (40, 10) and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.allclose(a.double().norm(dim=1), torch.ones(40, dtype=torch.float64), atol=1e-6)
    assert torch.equal(m._init_factors(40, 10, None, device="cpu"), m._init_factors(40, 10, 0, device="cpu"))
    big = m._init_factors(4000, 16, 3, device="cpu").double() * 4.0        # a unit row of 16 N(0, 1) draws: elements ~ N(0, 1/16)
    assert abs(float(big.mean())) < 0.02 and abs(float(big.std()) - 1.0) < 0.03


def test_fit_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    log = pd.DataFrame({"user_idx": [0, 1], "item_idx": [0, 1], "relevance": [1.0, 1.0]})
    with pytest.raises(N.CqlrecError, match="no CPU path"):
        ALS.ALSWrap().fit(log)


def test_count_pieces():
    off = torch.tensor([0, 0, 1024, 2049, 2049 + 2051, 2049 + 2051 + 5])
    assert ALS.count_pieces(off) == 2 + 3                       # 1024 entries are one piece: not cut; 1025 -> 2; 2051 -> 3
    assert ALS.count_pieces(off, torch.tensor([3, 0], dtype=torch.int32)) == 3
    assert ALS.count_pieces(off, torch.tensor([1], dtype=torch.int32)) == 0


@pytest.mark.parametrize("fn", ["cqlrec_als_normal_equations_ws_bytes", "cqlrec_als_half_step_ws_bytes"])
def test_row_workspace_is_monotone_and_per_piece(lib, fn):
    f = getattr(lib, fn)
    assert len(N.SIGNATURES[fn][1]) == 3                          # (n_list, n_pieces, rank): no argument for the source side
    ranks = list(range(1, 129))
    for n_list, n_pieces in ((1, 0), (60, 5), (100000, 300)):
        sizes = [f(n_list, n_pieces, r) for r in ranks]
        assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert f(n_list + 1000, n_pieces, 10) >= f(n_list, n_pieces, 10)
        assert f(n_list, n_pieces + 1, 10) > f(n_list, n_pieces, 10)
    for r in (1, 10, 33, 64, 128):                               # every further piece costs the same, and holds the triangle
        step = f(60, 6, r) - f(60, 5, r)
        assert abs(step - (f(60, 50, r) - f(60, 49, r))) <= 512          # sections are rounded to 256 bytes
        assert step >= (r + 1) * (r + 2) // 2 * 8 - 256
    for bad in ((-1, 0, 10), (5, -1, 10), (5, 0, 0), (5, 0, 129), (1 << 31, 0, 10)):
        assert f(*bad) == 0


def test_gram_workspace(lib):
    f = lib.cqlrec_als_gram_ws_bytes
    sizes = [f(n, 128) for n in (0, 1, 4096, 4097, 10 ** 5, 10 ** 6)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert f(4096, 128) == f(0, 128) < f(4097, 128)               # up to one block of rows there is no partial matrix
    assert all(f(10 ** 6, a) <= f(10 ** 6, a + 1) for a in range(1, 128))
    assert f(10, 0) == 0 and f(10, 129) == 0 and f(-1, 10) == 0


def test_argument_validation_without_gpu(lib):
    """validation happens on the host before any HIP call"""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    with pytest.raises(N.CqlrecError, match=r"rank=129 out of range \(rank 1..128\)"):
        N.check(lib.cqlrec_als_gram(p, 4, 129, p, 1 << 20, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_als_gram(p, 4, 8, p, 1 << 20, None, None))
    with pytest.raises(N.CqlrecError, match="workspace"):
        N.check(lib.cqlrec_als_gram(p, 4, 8, p, 16, p, None))
    with pytest.raises(N.CqlrecError, match="rank=0 out of range"):
        N.check(lib.cqlrec_als_half_step(p, p, p, 2, p, 2, 0, p, 1, 1.0, 0.1, None, 2, 0, p, 1 << 24, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="unknown mode 2"):
        N.check(lib.cqlrec_als_half_step(p, p, p, 2, p, 2, 4, p, 2, 1.0, 0.1, None, 2, 0, p, 1 << 24, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="reg=-1 must be non-negative"):
        N.check(lib.cqlrec_als_half_step(p, p, p, 2, p, 2, 4, p, 1, 1.0, -1.0, None, 2, 0, p, 1 << 24, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="alpha"):
        N.check(lib.cqlrec_als_half_step(p, p, p, 2, p, 2, 4, p, 1, float("nan"), 0.1, None, 2, 0, p, 1 << 24, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="implicit mode needs G"):
        N.check(lib.cqlrec_als_half_step(p, p, p, 2, p, 2, 4, None, 1, 1.0, 0.1, None, 2, 0, p, 1 << 24, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="n_list must be n_dst"):
        N.check(lib.cqlrec_als_half_step(p, p, p, 2, p, 2, 4, p, 1, 1.0, 0.1, None, 1, 0, p, 1 << 24, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="workspace holds 16 bytes"):
        N.check(lib.cqlrec_als_half_step(p, p, p, 2, p, 2, 4, p, 1, 1.0, 0.1, None, 2, 0, p, 16, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_als_normal_equations(p, p, p, 2, p, 2, 4, p, 1, 1.0, None, 2, 0, p, 1 << 24, p, None, p, None))
    assert lib.cqlrec_als_half_step(None, None, None, 0, None, 0, 4, None, 0, 1.0, 0.1, None, 0, 0, None, 0, None, None, None,
                                    None) == 0                    # nothing listed: nothing to do
    with pytest.raises(N.CqlrecError, match=r"k=513 out of range \(1..512\)"):
        N.check(lib.cqlrec_als_topk(p, 1, p, p, 1, p, p, 1, 4, None, None, None, 513, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="k=0 out of range"):
        N.check(lib.cqlrec_als_topk(p, 1, p, p, 1, p, p, 1, 4, None, None, None, 0, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="both arrays"):
        N.check(lib.cqlrec_als_topk(p, 1, p, p, 1, p, p, 1, 4, None, p, None, 5, p, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_als_topk(p, 1, p, p, 1, p, p, 1, 4, None, None, None, 5, None, p, p, None))
    with pytest.raises(N.CqlrecError, match="rank=200"):
        N.check(lib.cqlrec_als_pair_scores(p, p, 1, p, p, 1, p, p, 1, 200, p, p, None))
    with pytest.raises(N.CqlrecError, match="NULL"):
        N.check(lib.cqlrec_als_pair_scores(p, p, 1, p, p, 1, p, p, 1, 4, None, p, None))
    assert lib.cqlrec_als_pair_scores(None, None, 0, None, None, 0, None, None, 0, 4, None, None, None) == 0
