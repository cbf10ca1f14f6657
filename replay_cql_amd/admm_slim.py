"""ADMM SLIM on the device: `ADMMSLIM` (replay/models/admm_slim.py) over csrc/dense.hip (section f11 of
include/cqlrec.h).  DESIGN.md section 3.14 is the normative text.

`fit` is dense fp64 linear algebra on n = n_items: the Gram matrix G = X^T X of the log (duplicated (user, item) rows
summed), W = (G + (lambda_2 + rho_0) I)^-1 by a blocked Cholesky factorisation, P = W G, and up to `max_iteration` ADMM
iterations, each one n x n x n product on the fp64 matrix pipe with the element-wise update fused behind it.  rho, its
branch and the stopping test live on the host: five sums of squares come back per iteration.  The similarity table is
the non-zeros of the final C as CSR -- a row can be n wide, so the padded [n_items, K] table of the other neighbourhood
models does not fit (`_similarity.Csr`); `predict`, `predict_pairs`, `recommend` and `get_nearest_items` are
`NeighbourRec`'s.
The engine class `Dense` and the front of the fit, from the log to G, are `_dense.py`'s, shared with slim.py.

The starting matrices are drawn on the HOST from numpy.random.RandomState(seed), B, C, Gamma in the reference's order,
and uploaded: a seeded fit is comparable with the reference's, at the price of 3 n^2 host draws and 16 n^2 bytes over
the bus.  Deviation from the reference, stated in DESIGN.md section 3.14: every `fit` starts from rho = lambda_2 (the
reference starts a second fit from the rho the first one ended with); `rho` holds the last value afterwards.

Nothing here has a CPU path: without a GPU every call that computes raises CqlrecError."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._dense import Dense
from ._similarity import Csr
from .neighbour import NeighbourRec

__all__ = ["ADMMSLIM"]

_DRAW_CHUNK = 1 << 22                  # doubles of the discarded draw held at once


class ADMMSLIM(NeighbourRec):
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
        G, n, _ = D.log_gram(lg, "admm_iteration",
                             "ADMMSLIM holds dense n_items x n_items matrices: {n} items are out of range")
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
        self._sim = Csr(*D.to_csr(C))
        self.rho, self.rho_sequence, self.n_iterations = rho, rhos, it
        self.residuals = (r_p, r_d, e_p, e_d)
