"""The calls into csrc/dense.hip (section f11 of include/cqlrec.h) that the models fitted on the Gram matrix of the log
share (admm_slim.py, slim.py), and the front of their fits: from the log to G = X^T X."""
from __future__ import annotations

from typing import Optional

import torch

from . import _prepare as P
from ._device import Ws
from ._log import dense_ids, float_column, has_column


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
        n_pieces = P.count_pieces(i_off, piece=self.N.DENSE_GRAM_PIECE)
        G = torch.empty((n_items, n_items), dtype=torch.float64, device=self.dev)
        self.call("dense_gram", i_off, i_user, i_val, u_off, u_item, u_val, int(n_items), int(n_users), n_pieces,
                  Ws(int(n_items), n_pieces), G)
        return G

    def log_gram(self, lg, ws_entry: str, out_of_range: str):
        """(G, n_items, n_users) of an opened log, duplicated (user, item) rows summed; the weight of a row is its
        relevance, or 1 without that column.  ValueError(out_of_range.format(n=n_items)) where the model's own workspace
        query `ws_entry` refuses n_items."""
        (user, n_users), (item, n_items) = dense_ids(lg, ["user_idx", "item_idx"])
        if has_column(lg.src, "relevance"):
            rel = float_column(lg, "relevance")
            if not bool(torch.isfinite(rel).all()):
                raise ValueError("relevance contains NaN or an infinite value")
        else:
            rel = torch.ones(user.numel(), dtype=torch.float64, device=lg.device)
        n = int(n_items)
        if self.ws_bytes(ws_entry, n) == 0:
            raise ValueError(out_of_range.format(n=n))
        item_view, _ = self.view(item, n_items, user, rel)
        user_view, _ = self.view(user, n_users, item, rel)
        return self.gram(item_view, user_view, n, n_users), n, int(n_users)

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
