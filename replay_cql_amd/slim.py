"""SLIM on the device: `SLIM` (replay/models/slim.py) over csrc/slim.hip (section f12 of include/cqlrec.h).  DESIGN.md
section 3.15 is the normative text.

Per target item j the reference fits sklearn's `ElasticNet(alpha = beta + lambda_, l1_ratio = lambda_ / alpha,
positive=True, fit_intercept=False)` of column j of the interaction matrix on the other columns:

    min over w >= 0, w_j = 0 of   1/(2 n_users) |x_j - X w|^2 + lambda_ |w|_1 + beta/2 |w|^2

With beta > 0 the minimiser is unique whatever order the coordinates are visited in, so the fit here is pinned to the
MINIMISER, not to sklearn's randomly ordered iterates: `fit` is the Gram matrix G = X^T X of the log (duplicated (user,
item) rows summed), one cyclic coordinate descent per column on G (`cqlrec_slim_fit`), and the non-zeros of the result
as CSR.  Every column carries its own certificate, the largest violation of the optimality (KKT) conditions, in `kkt`.

Deviations from the reference, stated in DESIGN.md section 3.15: `seed` is kept and returned but has no effect, the fit
is deterministic; `tol` is sklearn's default NUMBER (1e-4) under OUR criterion, certificate <= tol * lambda_, where
sklearn compares a dual gap scaled by |x_j|^2; `max_iter` counts full ascending sweeps.

Nothing here has a CPU path: without a GPU every call that computes raises CqlrecError."""
from __future__ import annotations

import warnings
from typing import Optional

import torch

from ._dense import Dense
from ._device import Ws
from ._similarity import Csr
from .neighbour import NeighbourRec

__all__ = ["SLIM"]


class SLIM(NeighbourRec):
    """SLIM: Sparse Linear Methods for Top-N Recommender Systems (Ning and Karypis, ICDM 2011)."""

    tol: float = 1.0e-4            # a column is done at certificate <= tol * lambda_ (not sklearn's dual-gap rule)
    max_iter: int = 5000           # full sweeps per column, the reference's number
    _search_space = {
        "beta": {"type": "loguniform", "args": [1e-6, 5]},
        "lambda_": {"type": "loguniform", "args": [1e-6, 2]},
    }

    def __init__(self, beta: float = 0.01, lambda_: float = 0.01, seed: Optional[int] = None):
        """beta: l2 regularization; lambda_: l1 regularization; seed: kept for the reference's signature and returned by
        `_init_args`, unused -- the fit is deterministic"""
        if beta < 0 or lambda_ <= 0:
            raise ValueError("Invalid regularization parameters")
        self.beta = beta
        self.lambda_ = lambda_
        self.seed = seed

    @property
    def _init_args(self):
        return {"beta": self.beta, "lambda_": self.lambda_, "seed": self.seed}

    def solve(self, D: Dense, G, n_users: int, col_begin: int = 0, col_end: Optional[int] = None, S=None):
        """(S, sweeps, kkt, updates) of `cqlrec_slim_fit` on the columns [col_begin, col_end) of the Gram matrix G; the
        other columns of S and the other entries of the three vectors are zero (or what `S` held)"""
        n = int(G.shape[0])
        col_end = n if col_end is None else int(col_end)
        S = torch.zeros((n, n), dtype=torch.float64, device=D.dev) if S is None else S
        sweeps = torch.zeros(n, dtype=torch.int32, device=D.dev)
        kkt = torch.zeros(n, dtype=torch.float64, device=D.dev)
        updates = torch.zeros(n, dtype=torch.int64, device=D.dev)
        D.call("slim_fit", G, max(int(G.stride(0)), n) if n > 1 else n, n, int(n_users), float(self.beta), float(self.lambda_),
               float(self.tol), int(self.max_iter), int(col_begin), col_end, Ws(n), S, n, sweeps, kkt, updates)
        return S, sweeps, kkt, updates

    def _fit_device(self, lg) -> None:
        D = Dense(lg.device)
        G, n, n_users = D.log_gram(lg, "slim_fit", "SLIM holds a dense n_items x n_items matrix and one column in the LDS: "
                                   "{n} items are out of range")
        S, sweeps, kkt, updates = self.solve(D, G, n_users)
        del G
        self._clear_cache()
        self._sim = Csr(*D.to_csr(S))
        self.n_sweeps, self.kkt = sweeps, kkt
        self.n_updates = int(updates.sum().item())
        self.n_not_converged = int((kkt > float(self.tol) * float(self.lambda_)).sum().item())
        if self.n_not_converged:
            warnings.warn(f"SLIM: {self.n_not_converged} of {n} columns did not reach the certificate "
                          f"{float(self.tol) * float(self.lambda_):g} within {int(self.max_iter)} sweeps; consider a larger "
                          "max_iter or a larger regularisation", RuntimeWarning, stacklevel=3)
