"""`ALSWrap` (replay/models/als.py) on the device, over csrc/als.hip (section f9 of include/cqlrec.h).

The reference wraps Spark ML's ALS; this package owns the solver.  DESIGN.md section 3.10 is the normative text of the
algorithm -- Spark ML ALS at the settings the wrapper uses (maxIter = 10, regParam = 0.1, alpha = 1, nonnegative = False,
coldStartStrategy = "drop") -- and of what differs: the initial draw is this package's counter-based generator, not
Spark's XORShift stream, so factors agree with a Spark run in distribution and objective, not element by element.

The two CSR views of the log come from cqlrec_features_segments: rows by (item, user, row) for the item step and by
(user, item, row) for the user step; duplicated (user, item) rows stay separate entries.  An id of the dense range
without a row in the log has no factor: it is absent from every prediction, as the reference's "drop" has it.

Nothing here has a CPU path: without a GPU every call that computes raises CqlrecError."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import pandas as pd
import torch

from . import _log as L
from . import _prepare as P
from . import data as D
from ._device import Ws
from ._prepare import count_pieces
from .device_recommender import DeviceRecommender

__all__ = ["ALSWrap"]

MAX_RANK, MAX_K, PIECE = 128, 512, 1024


class Als(P.Feat):
    """The calls into csrc/als.hip on one device.  A side = (offsets int64 [n_dst + 1], src int32 [nnz], rating float64
    [nnz]) in the order of `segments`."""

    def gram(self, F):
        n, r = F.shape
        G = torch.empty((r, r), dtype=torch.float64, device=self.dev)
        self.call("als_gram", F, n, r, Ws(n, r), G)
        return G

    def _mode(self, implicit: bool) -> int:
        return self.N.ALS_IMPLICIT if implicit else self.N.ALS_EXPLICIT

    def normal_equations(self, side, F, G, implicit: bool, alpha: float, rows=None, n_pieces: Optional[int] = None):
        """(A float64 [n_list, r, r] with G but without the regulariser, b float64 [n_list, r], n_expl int32 [n_list])"""
        off, src, rating = side
        n_dst, (n_src, r) = off.numel() - 1, F.shape
        n_list = n_dst if rows is None else rows.numel()
        n_pieces = count_pieces(off, rows) if n_pieces is None else int(n_pieces)
        A = torch.empty((n_list, r, r), dtype=torch.float64, device=self.dev)
        b = torch.empty((n_list, r), dtype=torch.float64, device=self.dev)
        ne = self._empty(n_list, torch.int32)
        self.call("als_normal_equations", off, src, rating, n_dst, F, n_src, r, G, self._mode(implicit), float(alpha), rows,
                  n_list, n_pieces, Ws(n_list, n_pieces, r), A, b, ne)
        return A, b, ne

    def half_step(self, side, F, G, implicit: bool, alpha: float, reg: float, X, has, failed, rows=None,
                  n_pieces: Optional[int] = None) -> None:
        """the listed rows of X float32 [n_dst, r] and has uint8 [n_dst] in place; `failed` int32 [1] is added to"""
        off, src, rating = side
        n_dst, (n_src, r) = off.numel() - 1, F.shape
        if X.shape != (n_dst, r) or has.numel() != n_dst:
            raise ValueError("X / has_factor do not have one row per destination row")
        n_list = n_dst if rows is None else rows.numel()
        n_pieces = count_pieces(off, rows) if n_pieces is None else int(n_pieces)
        self.call("als_half_step", off, src, rating, n_dst, F, n_src, r, G, self._mode(implicit), float(alpha), float(reg),
                  rows, n_list, n_pieces, Ws(n_list, n_pieces, r), X, has, failed)

    def topk(self, users, U, u_has, V, v_has, k: int, mask=None, seen=None):
        """(ids int32 [n_q, k] padded with -1, values float32 [n_q, k] padded with -inf, count int32 [n_q]); seen =
        (offsets int64 [>= n_users + 1] indexed by the user id, ascending item ids)"""
        n_q, (n_users, r), n_items = users.numel(), U.shape, V.shape[0]
        ids = torch.empty((n_q, k), dtype=torch.int32, device=self.dev)
        vals = torch.empty((n_q, k), dtype=torch.float32, device=self.dev)
        count = self._empty(n_q, torch.int32)
        s_off, s_col = seen if seen is not None else (None, None)
        if s_off is not None and s_off.numel() < n_users + 1:
            raise ValueError("the seen lists need an offset per user")
        self.call("als_topk", users, n_q, U, u_has, n_users, V, v_has, n_items, r, mask, s_off, s_col, int(k), ids, vals, count)
        return ids, vals, count

    def pair_scores(self, pair_user, pair_item, U, u_has, V, v_has):
        """(score float32 [n_pairs], valid uint8 [n_pairs])"""
        n = pair_user.numel()
        score, valid = self._empty(n, torch.float32), self._empty(n, torch.uint8)
        self.call("als_pair_scores", pair_user, pair_item, n, U, u_has, U.shape[0], V, v_has, V.shape[0], U.shape[1], score,
                  valid)
        return score, valid


class ALSWrap(DeviceRecommender):
    """Alternating least squares for implicit (default) or explicit feedback.

    `_predict` returns at most k rows per user, already without the seen items and without ids that have no factor; the
    template's `_filter_seen` and `get_top_k_recs` then change nothing, as with `NeighbourRec`."""

    _seed: Optional[int] = None
    _state_attr = "_factors"
    _search_space = {"rank": {"type": "loguniform_int", "args": [8, 256]}}

    def __init__(self, rank: int = 10, implicit_prefs: bool = True, seed: Optional[int] = None, *, max_iter: int = 10,
                 reg_param: float = 0.1, alpha: float = 1.0):
        """rank: hidden dimension, 1..128; implicit_prefs: implicit feedback; seed: of the initial user factors (None: 0).
        max_iter, reg_param and alpha are Spark ML's maxIter, regParam and alpha at the values the reference leaves them."""
        if isinstance(rank, bool) or int(rank) != rank or not 1 <= int(rank) <= MAX_RANK:
            raise ValueError(f"rank must be an integer in 1..{MAX_RANK}, got {rank}")
        if int(max_iter) < 0 or not float(reg_param) >= 0.0 or not float(alpha) >= 0.0:
            raise ValueError("max_iter, reg_param and alpha must be non-negative")
        self.rank = int(rank)
        self.implicit_prefs = bool(implicit_prefs)
        self._seed = seed
        self.max_iter, self.reg_param, self.alpha = int(max_iter), float(reg_param), float(alpha)

    @property
    def _init_args(self):
        return {"rank": self.rank, "implicit_prefs": self.implicit_prefs, "seed": self._seed}

    # -------------------------------------------------------------------------------- fit
    def _init_factors(self, n: int, rank: int, seed: Optional[int], device=None) -> torch.Tensor:
        """float32 [n, rank]: N(0, 1) per element by Box-Muller from the counter-based generator of `data` (element e =
        row * rank + column draws from _mix64(e ^ seed * 0x2545F491) and the mix of that), each row scaled to unit L2
        norm in float64 and rounded to float32.  The draw is this package's own: Spark seeds an XORShift stream."""
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        e = torch.arange(int(n) * int(rank), dtype=torch.int64, device=dev)
        h = D._mix64(e ^ (int(seed or 0) * 0x2545F491))
        z = torch.sqrt(-2.0 * torch.log(D._u01(h))) * torch.cos(2.0 * math.pi * D._u01(D._mix64(h)))
        z = z.reshape(int(n), int(rank))
        norm = torch.sqrt((z * z).sum(dim=1, keepdim=True))
        return (z / norm).to(torch.float32).contiguous()

    def _fit_device(self, lg) -> None:
        if lg.n == 0:
            raise ValueError("cannot fit an empty log")
        eng = Als(lg.device)
        (user, n_users), (item, n_items) = L.dense_ids(lg, ["user_idx", "item_idx"])
        rel = L.float_column(lg, "relevance")
        if bool(torch.isnan(rel).any()):
            raise ValueError("relevance contains NaN")
        item_side, _ = eng.view(item, n_items, user, rel)
        user_side, _ = eng.view(user, n_users, item, rel)
        off_u = user_side[0]
        np_i, np_u = count_pieces(item_side[0]), count_pieces(off_u)
        r, dev = self.rank, lg.device
        U = self._init_factors(n_users, r, self._seed, dev)
        U = (U * (off_u[1:] > off_u[:-1]).to(torch.float32)[:, None]).contiguous()     # an id without rows has a zero row
        V = torch.zeros((n_items, r), dtype=torch.float32, device=dev)
        has_u = (off_u[1:] > off_u[:-1]).to(torch.uint8)
        has_v = torch.zeros(n_items, dtype=torch.uint8, device=dev)
        failed = torch.zeros(1, dtype=torch.int32, device=dev)
        imp = self.implicit_prefs
        for _ in range(self.max_iter):
            eng.half_step(item_side, U, eng.gram(U) if imp else None, imp, self.alpha, self.reg_param, V, has_v, failed,
                          n_pieces=np_i)
            eng.half_step(user_side, V, eng.gram(V) if imp else None, imp, self.alpha, self.reg_param, U, has_u, failed,
                          n_pieces=np_u)
        n_failed = int(failed.item())
        if n_failed:
            raise ValueError(f"{self}: {n_failed} normal equations were not positive definite (a singular system: "
                             "raise reg_param)")
        self._factors = {"user": (U, has_u), "item": (V, has_v)}

    # -------------------------------------------------------------------------------- the tables
    def factors_device(self, entity: str):
        """(factors float32 [n, rank], has_factor uint8 [n]) of 'user' or 'item' on the device, indexed by the id"""
        if entity not in ("user", "item"):
            raise ValueError("entity must be 'user' or 'item'")
        return self._fitted()[entity]

    # -------------------------------------------------------------------------------- predict on the device
    def _recommend(self, log, k: int, users, items, filter_seen_items: bool):
        """(users int64 [m], ids int32 [m, k], values float32 [m, k], count int32 [m]) on the device"""
        (U, has_u), (V, has_v) = self._fitted()["user"], self._fitted()["item"]
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
        dev = U.device
        eng = Als(dev)
        lg = None
        if log is not None:
            lg = L.open_log(L.normalise(log), str(self))
            if lg.device != dev:
                raise ValueError(f"the log is on {lg.device}, the model on {dev}")
        users, items = self._id_tensor(users, dev), self._id_tensor(items, dev)
        seen = None
        if lg is not None and lg.n:
            (user, n_log_users), (item, _) = L.dense_ids(lg, ["user_idx", "item_idx"])
            if users is None:
                users = torch.unique(user.to(torch.int64))
            if filter_seen_items:
                n_rows = max(n_log_users, U.shape[0])
                (off, seen_items, _), _ = eng.view(user, n_rows, item)
                seen = (off, seen_items)
        if users is None:
            users = torch.nonzero(has_u).flatten()
        users = users[users < (1 << 31) - 1]
        mask = self._item_mask(items, V.shape[0], dev)
        ids, vals, count = eng.topk(users.to(torch.int32).contiguous(), U, has_u, V, has_v, int(k), mask=mask, seen=seen)
        return users, ids, vals, count

    def _predict_pairs(self, pairs: pd.DataFrame, log=None, user_features=None, item_features=None) -> pd.DataFrame:
        (U, has_u), (V, has_v) = self._fitted()["user"], self._fitted()["item"]
        pu_h, pi_h = pairs["user_idx"].to_numpy().astype(np.int64), pairs["item_idx"].to_numpy().astype(np.int64)
        lim = (1 << 31) - 1
        pu = torch.as_tensor(np.where((pu_h >= 0) & (pu_h < lim), pu_h, -1).astype(np.int32), device=U.device)
        pi = torch.as_tensor(np.where((pi_h >= 0) & (pi_h < lim), pi_h, -1).astype(np.int32), device=U.device)
        score, valid = Als(U.device).pair_scores(pu, pi, U, has_u, V, has_v)
        keep = valid.bool().cpu().numpy()
        return pd.DataFrame({"user_idx": pu_h[keep].astype(np.int32), "item_idx": pi_h[keep].astype(np.int32),
                             "relevance": score.cpu().numpy()[keep].astype(np.float64)})

    # -------------------------------------------------------------------------------- features, vectors
    def _get_features(self, ids: pd.DataFrame, features):
        """(the right join of the factors on `ids`, rank): column `<entity>_factors` holds a list per id, None for an id
        without a factor (als.py:137-148)"""
        entity = "user" if "user_idx" in ids.columns else "item"
        F, has = self._fitted()[entity]
        col = ids[f"{entity}_idx"].to_numpy().astype(np.int64)
        ok = (col >= 0) & (col < F.shape[0])
        ok[ok] = has.cpu().numpy()[col[ok]] != 0
        rows = F[torch.as_tensor(col[ok], device=F.device)].cpu().numpy()
        vecs = np.empty(len(col), dtype=object)
        vecs[:] = None
        for pos, row in zip(np.nonzero(ok)[0], rows):
            vecs[pos] = row.tolist()
        out = ids.reset_index(drop=True).copy()
        out[f"{entity}_factors"] = vecs
        return out, self.rank

    def _get_item_vectors(self) -> pd.DataFrame:
        """[item_idx, item_vector] of the items that have a factor (als.py:150-154)"""
        V, has = self._fitted()["item"]
        idx = torch.nonzero(has).flatten()
        return pd.DataFrame({"item_idx": idx.cpu().numpy().astype(np.int32), "item_vector": list(V[idx].cpu().numpy())})

    # -------------------------------------------------------------------------------- persistence
    def _save_model(self, path: str) -> None:
        (U, has_u), (V, has_v) = self._fitted()["user"], self._fitted()["item"]
        # tensors, numbers and strings only: the file loads with weights_only=True (nothing in it is executed)
        torch.save({"user_factors": U.cpu(), "user_has": has_u.cpu(), "item_factors": V.cpu(), "item_has": has_v.cpu(),
                    "init_args": {"rank": self.rank, "implicit_prefs": self.implicit_prefs,
                                  "seed": -1 if self._seed is None else int(self._seed), "has_seed": self._seed is not None},
                    "solver": {"max_iter": self.max_iter, "reg_param": self.reg_param, "alpha": self.alpha},
                    "fit": {"users": torch.as_tensor(self.fit_users["user_idx"].to_numpy().astype(np.int64)),
                            "items": torch.as_tensor(self.fit_items["item_idx"].to_numpy().astype(np.int64)),
                            "user_dim": int(self._user_dim_size), "item_dim": int(self._item_dim_size)}}, path)

    def _load_model(self, path: str, device=None) -> None:
        from ._native import CqlrecError
        if not torch.cuda.is_available():
            raise CqlrecError(f"{self} needs a GPU: it has no CPU path")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        blob = torch.load(path, weights_only=True, map_location="cpu")
        a = blob["init_args"]
        self.rank, self.implicit_prefs = int(a["rank"]), bool(a["implicit_prefs"])
        self._seed = int(a["seed"]) if a["has_seed"] else None
        s = blob["solver"]
        self.max_iter, self.reg_param, self.alpha = int(s["max_iter"]), float(s["reg_param"]), float(s["alpha"])
        self._factors = {"user": (blob["user_factors"].to(dev).contiguous(), blob["user_has"].to(dev).contiguous()),
                         "item": (blob["item_factors"].to(dev).contiguous(), blob["item_has"].to(dev).contiguous())}
        f = blob["fit"]
        self.fit_users = pd.DataFrame({"user_idx": f["users"].numpy()})
        self.fit_items = pd.DataFrame({"item_idx": f["items"].numpy()})
        self._num_users, self._num_items = len(self.fit_users), len(self.fit_items)
        self._user_dim_size, self._item_dim_size = int(f["user_dim"]), int(f["item_dim"])
