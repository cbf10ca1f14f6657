"""ADMM SLIM on the device: `ADMMSLIM` (replay/models/admm_slim.py) over csrc/dense.hip (section f11 of
include/cqlrec.h).  DESIGN.md section 3.14 is the normative text.

`fit` is dense fp64 linear algebra on n = n_items: the Gram matrix G = X^T X of the log (duplicated (user, item) rows
summed), W = (G + (lambda_2 + rho_0) I)^-1 by a blocked Cholesky factorisation, P = W G, and up to `max_iteration` ADMM
iterations, each one n x n x n product on the fp64 matrix pipe with the element-wise update fused behind it.  rho, its
branch and the stopping test live on the host: five sums of squares come back per iteration.  The similarity table is
the non-zeros of the final C as CSR -- a row can be n wide, so the padded [n_items, K] table of the other neighbourhood
models does not fit; `predict`, `predict_pairs`, `recommend` and `get_nearest_items` are `NeighbourRec`'s.

The starting matrices are drawn on the HOST from numpy.random.RandomState(seed), B, C, Gamma in the reference's order,
and uploaded: a seeded fit is comparable with the reference's, at the price of 3 n^2 host draws and 16 n^2 bytes over
the bus.  Deviation from the reference, stated in DESIGN.md section 3.14: every `fit` starts from rho = lambda_2 (the
reference starts a second fit from the rho the first one ended with); `rho` holds the last value afterwards.

Nothing here has a CPU path: without a GPU every call that computes raises CqlrecError."""
from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import pandas as pd
import torch

from . import _prepare as P
from ._device import Ws
from ._log import dense_ids, float_column, has_column
from .neighbour import NeighbourRec

__all__ = ["ADMMSLIM"]

_DRAW_CHUNK = 1 << 22                  # doubles of the discarded draw held at once


class Dense(P.Feat):
    """The calls into csrc/dense.hip on one device."""

    def gemm(self, A, B, E=None, alpha: float = 1.0, beta: float = 0.0, trans_a: bool = False, trans_b: bool = False, out=None):
        """alpha op(A) op(B) + beta E for 2-D float64 tensors whose rows are contiguous (a column slice of a wider matrix
        is taken with its leading dimension)"""
        m, k = (A.shape[1], A.shape[0]) if trans_a else A.shape
        n = B.shape[0] if trans_b else B.shape[1]
        if (B.shape[1] if trans_b else B.shape[0]) != k or (E is not None and tuple(E.shape) != (m, n)):
            raise ValueError("gemm: the shapes do not fit")
        out = torch.empty((m, n), dtype=torch.float64, device=self.dev) if out is None else out
        for t in (A, B, E, out):
            if t is not None and (t.dtype != torch.float64 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1)):
                raise ValueError("gemm: 2-D float64 tensors with contiguous rows are expected")
        ld = lambda t: max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])   # noqa: E731
        self.call("dense_gemm_f64", A, ld(A), int(trans_a), B, ld(B), int(trans_b), E, ld(E) if E is not None else 0,
                  float(alpha), float(beta), int(m), int(n), int(k), out, ld(out))
        return out

    def gram(self, item_view, user_view, n_items: int, n_users: int):
        """G [n_items, n_items] = X^T X from the two CSR views (offsets, ids, values) of a log"""
        i_off, i_user, i_val = item_view
        u_off, u_item, u_val = user_view
        piece = self.N.DENSE_GRAM_PIECE
        lens = i_off[1:] - i_off[:-1]
        n_pieces = int(torch.where(lens > piece, (lens + piece - 1) // piece, torch.zeros_like(lens)).sum().item())
        G = torch.empty((n_items, n_items), dtype=torch.float64, device=self.dev)
        self.call("dense_gram", i_off, i_user, i_val, u_off, u_item, u_val, int(n_items), int(n_users), n_pieces,
                  Ws(int(n_items), n_pieces), G)
        return G

    def spd_inverse(self, A, shift: float = 0.0):
        """(A + shift I)^-1 of a symmetric positive definite matrix; ValueError when a pivot is not positive"""
        n = int(A.shape[0])
        X = torch.empty((n, n), dtype=torch.float64, device=self.dev)
        status = self._empty(1, torch.int32)
        self.call("dense_spd_inverse", A, max(int(A.stride(0)), n) if n > 1 else n, n, float(shift), Ws(n), X, status)
        bad = int(status.item())
        if bad:
            raise ValueError(f"the matrix is not positive definite: pivot {bad - 1} of its Cholesky factorisation is not positive")
        return X

    def admm_iteration(self, W, Pm, C, Gamma, rho: float, lambda_1: float, ws, sums):
        n = int(W.shape[0])
        self.call("admm_iteration", W, Pm, C, Gamma, n, float(rho), float(lambda_1), ws, int(ws.numel()), sums)

    def to_csr(self, C, n_rows: Optional[int] = None):
        """(offsets int64 [n_rows + 1], columns int32 ascending, values float64) of the non-zeros of C [n, n]"""
        n = int(C.shape[0])
        n_rows = n if n_rows is None else int(n_rows)
        off = self._empty(n_rows + 1, torch.int64)
        self.call("admm_compact", C, n, n_rows, off, None, None)
        nnz = int(off[n].item())
        col, val = self._empty(nnz, torch.int32), self._empty(nnz, torch.float64)
        if nnz:
            self.call("admm_compact", C, n, n_rows, off, col, val)
        return off, col, val


class CsrTable:
    """The similarity table of a model whose `_sim` is a CSR triple of an n_items x n_items matrix (ADMMSLIM, SLIM), as
    `NeighbourRec` reads it; listed in front of `NeighbourRec` among the bases."""

    @property
    def similarity_device(self):
        """the CSR triple (offsets int64 [n_items + 1], item_idx_two int32 ascending inside a row, similarity float64) on
        the device -- NOT the padded (ids, values, counts) of the other neighbourhood models: row i holds the non-zeros
        of row i of the fitted matrix"""
        return self._fitted()

    def _n_rows(self) -> int:
        return int(self._fitted()[0].numel()) - 1

    def _csr(self, n_rows: int):
        """the table with n_rows >= n_items rows; the columns of a row ascend, so one CSR serves both readers"""
        cache = self.__dict__.setdefault("_csr_cache", {})
        if n_rows not in cache:
            off, col, val = self._fitted()
            if n_rows + 1 > off.numel():
                off = torch.cat([off, off[-1:].expand(n_rows + 1 - off.numel())])
            cache.clear()
            cache[n_rows] = ((off, col, val), (off, col, val))
        return cache[n_rows]

    @property
    def similarity(self) -> pd.DataFrame:
        """[item_idx_one, item_idx_two, similarity]: the non-zeros of the fitted matrix, row-major"""
        if "_similarity_frame" not in self.__dict__:
            off, col, val = self._fitted()
            lens = (off[1:] - off[:-1]).cpu().numpy()
            self._similarity_frame = pd.DataFrame({"item_idx_one": np.repeat(np.arange(len(lens), dtype=np.int32), lens),
                                                   "item_idx_two": col.cpu().numpy(), "similarity": val.cpu().numpy()})
        return self._similarity_frame

    @property
    def _dataframes(self) -> Dict[str, Any]:
        return {"similarity": self.similarity}


class ADMMSLIM(CsrTable, NeighbourRec):
    """ADMM SLIM: Sparse Recommendations for Many Users (Steck et al., WSDM 2020) -- SLIM's item-to-item weights with the
    zero diagonal as a constraint, found by the alternating direction method of multipliers."""

    rho: float
    threshold: float = 5
    multiplicator: float = 2
    eps_abs: float = 1.0e-3
    eps_rel: float = 1.0e-3
    max_iteration: int = 100
    _search_space = {
        "lambda_1": {"type": "loguniform", "args": [1e-9, 50]},
        "lambda_2": {"type": "loguniform", "args": [1e-9, 5000]},
    }

    def __init__(self, lambda_1: float = 5, lambda_2: float = 5000, seed: Optional[int] = None):
        """lambda_1: l1 regularization term; lambda_2: l2 regularization term; seed: of the starting matrices"""
        if lambda_1 < 0 or lambda_2 <= 0:
            raise ValueError("Invalid regularization parameters")
        self.lambda_1 = lambda_1
        self.lambda_2 = lambda_2
        self.rho = lambda_2
        self.seed = seed

    @property
    def _init_args(self):
        return {"lambda_1": self.lambda_1, "lambda_2": self.lambda_2, "seed": self.seed}

    # -------------------------------------------------------------------------------- fit
    def _draw(self, n: int, dev):
        """(C, Gamma) on the device: the second and third of three rand(n, n) draws; the first is made and dropped"""
        rs = np.random.RandomState(self.seed) if self.seed is not None else np.random.RandomState()
        left = n * n
        while left:
            take = min(left, _DRAW_CHUNK)
            rs.random_sample(take)
            left -= take
        return [torch.from_numpy(rs.rand(n, n)).to(dev) for _ in range(2)]

    def _fit_device(self, lg) -> None:
        D = Dense(lg.device)
        (user, n_users), (item, n_items) = dense_ids(lg, ["user_idx", "item_idx"])
        if has_column(lg.src, "relevance"):
            rel = float_column(lg, "relevance")
            if not bool(torch.isfinite(rel).all()):
                raise ValueError("relevance contains NaN or an infinite value")
        else:
            rel = torch.ones(user.numel(), dtype=torch.float64, device=lg.device)
        n = int(n_items)
        if D.ws_bytes("admm_iteration", n) == 0:
            raise ValueError(f"ADMMSLIM holds dense n_items x n_items matrices: {n} items are out of range")
        perm_i, off_i = D.segments(item, n_items, user.to(torch.int64))
        perm_u, off_u = D.segments(user, n_users, item.to(torch.int64))
        perm_i, perm_u = perm_i.long(), perm_u.long()
        G = D.gram((off_i, user[perm_i].contiguous(), rel[perm_i].contiguous()),
                   (off_u, item[perm_u].contiguous(), rel[perm_u].contiguous()), n, n_users)
        rho = float(self.lambda_2)
        W = D.spd_inverse(G, float(self.lambda_2) + rho)
        Pm = D.gemm(W, G)
        del G
        C, Gamma = self._draw(n, lg.device)
        ws = D._ws(D.ws_bytes("admm_iteration", n))
        sums = D._empty(5, torch.float64)
        r_p, r_d = float("inf"), float(torch.linalg.norm(rho * C).item())   # B differs from C with probability 1
        e_p = e_d = 0.0
        it, rhos = 0, [rho]
        while (r_p > e_p or r_d > e_d) and it < int(self.max_iteration):
            it += 1
            D.admm_iteration(W, Pm, C, Gamma, rho, float(self.lambda_1), ws, sums)
            s = np.sqrt(sums.cpu().numpy())              # |B - C'|, |C' - C|, |B|, |C'|, |Gamma'|
            r_p, r_d = float(s[0]), float(rho * s[1])
            e_p = self.eps_abs * n + self.eps_rel * max(float(s[2]), float(s[3]))
            e_d = self.eps_abs * n + self.eps_rel * float(s[4])
            if r_p > self.threshold * r_d:
                rho *= self.multiplicator
            elif self.threshold * r_p < r_d:
                rho /= self.multiplicator
            rhos.append(rho)
        self._clear_cache()
        self._sim = D.to_csr(C)
        self.rho, self.rho_sequence, self.n_iterations = rho, rhos, it
        self.residuals = (r_p, r_d, e_p, e_d)
