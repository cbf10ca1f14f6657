"""Neighbourhood models on the device: `NeighbourRec` (replay/models/base_rec.py:1433-1609) and `ItemKNN`
(replay/models/knn.py) over csrc/neighbour.hip (section f8 of include/cqlrec.h).

`fit` is C = A^T A with the k best per row and `predict` is R = B S with the k best unseen per row: one engine -- the
row-wise top-k of a sparse x sparse product -- with two epilogues, so the n_items x n_items matrix is never formed.  The
two CSR views of the log come from cqlrec_features_segments: rows by (user, item, row) and rows by (item, user, row);
duplicated (user, item) rows stay separate entries, as the reference's self-join keeps them.

Deviations from the reference, both stated in DESIGN.md section 3.9: a pair whose denominator norm * norm + shrink is 0
is dropped (the reference divides by zero), and predict breaks ties by item_idx ascending (the reference leaves them to
Spark; get_top_k_recs of this package uses the same rule).

Nothing here has a CPU path: without a GPU every call that computes raises CqlrecError."""
from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import pandas as pd
import torch

from . import _prepare as P
from ._device import Ws
from ._log import dense_ids, float_column, normalise, open_log
from ._similarity import Padded
from .device_recommender import DeviceRecommender

__all__ = ["NeighbourRec", "ItemKNN"]

DEFAULT_MAX_TUPLES = 1 << 27          # about 12 GB of workspace: 88 bytes per tuple, see cqlrec_neighbour_topk_ws_bytes


class Neigh(P.Feat):
    """The calls into csrc/neighbour.hip on one device."""

    def weights(self, user, item, relevance, ucount, icount, n_items: int, weighting, k1: float, b: float):
        n = user.numel()
        out = self._empty(n, torch.float64)
        self.call("neighbour_weights", user, item, relevance, ucount, icount, n, int(n_items),
                  self.N.NEIGHBOUR_WEIGHTINGS[weighting], float(k1), float(b), out)
        return out

    def norms(self, perm, offsets, w, n_groups: int):
        out = self._empty(n_groups, torch.float64)
        self.call("neighbour_norms", perm, offsets, w, perm.numel(), n_groups, out)
        return out

    def _count(self, L, R, n_mid: int, max_tuples: int):
        """The count pass of a product: (entry prefix, the row prefix on the host, total tuples, the largest row's, the
        tuples a chunk holds).  Sets `self.expansion` and `self.row_prefix`."""
        l_off, l_col, _ = L
        n_q, nnz = l_off.numel() - 1, l_col.numel()
        eprefix, rprefix, stats = self._empty(nnz + 1, torch.int64), self._empty(n_q + 1, torch.int64), self._empty(2, torch.int64)
        # the count's workspace is gone when `call` returns, before the top-k's is allocated: that bounds peak memory
        self.call("neighbour_count", l_off, l_col, n_q, nnz, R[0], n_mid, Ws(nnz), eprefix, rprefix, stats)
        total, largest = stats.cpu().tolist()
        host_prefix = rprefix.cpu()                      # the chunks are cut on the host: 8 (n_q + 1) bytes
        self.expansion, self.row_prefix = (int(total), int(largest)), host_prefix
        if int(max_tuples) < 1:
            raise ValueError(f"max_tuples must be positive, got {max_tuples}")
        max_tuples = max(1, min(int(max_tuples), int(total)))   # no workspace beyond the expansion; the result is the same
        return eprefix, host_prefix, int(total), int(largest), max_tuples

    def topk(self, mode: int, L, R, n_mid: int, n_cols: int, k: int, max_tuples: int, norm_q=None, norm_j=None,
             shrink: float = 0.0, mask=None, seen=None):
        """(ids int32 [n_q, k] padded with -1, vals float64 [n_q, k], count int32 [n_q]) of the product of the CSR
        matrices L and R = (offsets int64, columns int32, values float64); seen = (offsets, ascending columns) per row.
        `self.expansion` = (total tuples, the largest row's) of the call."""
        l_off, l_col, l_val = L
        r_off, r_col, r_val = R
        n_q, nnz = l_off.numel() - 1, l_col.numel()
        ids = torch.empty((n_q, k), dtype=torch.int32, device=self.dev)
        vals = torch.empty((n_q, k), dtype=torch.float64, device=self.dev)
        count = self._empty(n_q, torch.int32)
        self.expansion = (0, 0)
        if n_q == 0:
            return ids, vals, count
        eprefix, host_prefix, total, largest, max_tuples = self._count(L, R, n_mid, max_tuples)
        nb = self.ws_bytes("neighbour_topk", n_q, n_cols, int(max_tuples), int(largest), int(k))
        if nb == 0:
            raise ValueError(f"neighbour top-k: k={k} (1..{self.N.NEIGHBOUR_MAX_K}), max_tuples={max_tuples} or a row of "
                             f"{largest} tuples (below 2^31) is out of range")
        s_off, s_col = seen if seen is not None else (None, None)
        self.call("neighbour_topk", int(mode), l_off, l_col, l_val, n_q, nnz, r_off, r_col, r_val, n_mid, n_cols, eprefix,
                  host_prefix, int(max_tuples), int(largest), int(k), norm_q, norm_j, float(shrink), mask, s_off, s_col,
                  self._ws(nb) if total else None, nb, ids, vals, count)
        return ids, vals, count

    def rules_distinct(self, session, item, relevance, perm):
        """uint8 [n]: 1 at one row of every distinct (session, item[, relevance]); `perm` brings equal triples together"""
        keep = self._empty(session.numel(), torch.uint8)
        self.call("rules_distinct", session, item, relevance, perm, session.numel(), keep)
        return keep

    def rules_topk(self, L, R, n_sessions: int, k: int, max_tuples: int, num_sessions: int, min_pair_count: int):
        """(ids int32 [n_items, k] padded with -1, confidence, lift, confidence_gain float64 [n_items, k], count int32
        [n_items], item_relevance float64 [n_items]) of L = items x sessions and R = sessions x items (section f10)"""
        l_off, l_col, l_val = L
        r_off, r_col, r_val = R
        n_items, nnz = l_off.numel() - 1, l_col.numel()
        ids = torch.empty((n_items, k), dtype=torch.int32, device=self.dev)
        planes = [torch.empty((n_items, k), dtype=torch.float64, device=self.dev) for _ in range(3)]
        count, item_rel = self._empty(n_items, torch.int32), self._empty(n_items, torch.float64)
        self.expansion = (0, 0)
        if n_items == 0:
            return (ids, *planes, count, item_rel)
        eprefix, host_prefix, total, largest, max_tuples = self._count(L, R, n_sessions, max_tuples)
        nb = self.ws_bytes("rules_topk", n_items, max_tuples, largest, int(k))
        if nb == 0:
            raise ValueError(f"rules top-k: k={k} (1..{self.N.NEIGHBOUR_MAX_K}), max_tuples={max_tuples} or a row of "
                             f"{largest} tuples (below 2^31) is out of range")
        self.call("rules_topk", l_off, l_col, l_val, n_items, nnz, r_off, r_col, r_val, n_sessions, eprefix, host_prefix,
                  max_tuples, largest, int(k), int(num_sessions), int(min_pair_count), self._ws(nb) if total else None, nb,
                  ids, *planes, count, item_rel)
        return (ids, *planes, count, item_rel)

    def pair_scores(self, pair_user, pair_item, h_off, h_item, n_users: int, S, n_s_rows: int):
        """(score float64 [n_pairs], present uint8 [n_pairs]); S = a CSR whose rows are sorted by column"""
        s_off, s_col, s_val = S
        n = pair_user.numel()
        score, present = self._empty(n, torch.float64), self._empty(n, torch.uint8)
        self.call("neighbour_pair_scores", pair_user, pair_item, n, h_off, h_item, n_users, s_off, s_col, s_val, n_s_rows,
                  score, present)
        return score, present


class NeighbourRec(DeviceRecommender):
    """Base of the models that hold an item-to-item similarity table and need the log at prediction time.

    The score of (u, j) is the sum over the LOG ROWS (u, i) of S[i -> j]: duplicated rows count, the log's relevance does
    not enter, only j among `items` and only the users in `users` are scored; users without rows and rows whose item
    has no similarity row contribute nothing, so a user may get fewer than k rows, or none.

    `_predict` returns at most k rows per user, already without the user's seen items when `filter_seen_items` is set.
    The template's `_filter_seen` (the k + seen best, then an anti-join with the log) and `get_top_k_recs` (the k best by
    relevance descending, item_idx ascending) then change nothing: the first finds no seen pair among at most k rows,
    the second is handed at most k rows per user in exactly its own order."""

    can_predict_item_to_item: bool = True
    can_predict_cold_users: bool = True
    can_change_metric: bool = False
    item_to_item_metrics = ["similarity"]
    _similarity_metric = "similarity"
    max_tuples: int = DEFAULT_MAX_TUPLES
    _state_attr = "_sim"

    # -------------------------------------------------------------------------------- bookkeeping
    @property
    def _dataframes(self) -> Dict[str, Any]:
        return {"similarity": self.similarity}

    def _clear_cache(self) -> None:
        """the reference unpersists its cached frame; here the derived copies of the device table are dropped"""
        self.__dict__.pop("_similarity_frame", None)
        self.__dict__.pop("_csr_cache", None)

    @property
    def similarity_metric(self):
        return self._similarity_metric

    @similarity_metric.setter
    def similarity_metric(self, value):
        if not self.can_change_metric:
            raise ValueError("This class does not support changing similarity metrics")
        if value not in self.item_to_item_metrics:
            raise ValueError(f"Select one of the valid metrics for predict: {self.item_to_item_metrics}")
        self._similarity_metric = value

    # -------------------------------------------------------------------------------- the table
    @property
    def similarity_device(self):
        """the fitted table on the device, a tuple of tensors in one of the two formats of `_similarity`: `Padded` (ids,
        a value plane per measure, counts) or `Csr` (offsets, columns, values)"""
        return self._fitted()

    @property
    def similarity(self) -> pd.DataFrame:
        """[item_idx_one, item_idx_two, a column per measure], by item_idx_one ascending, then in the table's order"""
        if "_similarity_frame" not in self.__dict__:
            self._similarity_frame = self._fitted().frame()
        return self._similarity_frame

    def _n_rows(self) -> int:
        """the number of rows of the fitted table: one per item id below the largest fitted one + 1"""
        return self._fitted().n_rows

    def _csr(self, n_rows: int):
        """the table as CSR with n_rows >= n_items rows: (offsets, columns, values) in rank order, and sorted by column;
        the values are those of the current `similarity_metric`, and the cached copy follows a change of it"""
        cache = self.__dict__.setdefault("_csr_cache", {})
        key = (n_rows, self._similarity_metric)
        if key not in cache:
            cache.clear()
            cache[key] = self._fitted().csr(n_rows, self._similarity_metric)
        return cache[key]

    # -------------------------------------------------------------------------------- predict on the device
    def _history(self, lg):
        """(engine, users' CSR offsets, items of the rows ordered by (user, item, row), n_users, largest item + 1)"""
        (user, n_users), (item, n_items) = dense_ids(lg, ["user_idx", "item_idx"])
        eng = Neigh(lg.device)
        (off, h_item, _), _ = eng.view(user, n_users, item)
        return eng, off, h_item, n_users, n_items

    def _recommend(self, log, k: int, users, items, filter_seen_items: bool):
        """(users int64 [m], ids int32 [m, k], vals float64 [m, k], count int32 [m]) on the device"""
        n_cols = self._n_rows()
        if log is None:
            raise ValueError("log is not provided, but it is required for prediction")
        lg = open_log(normalise(log), str(self))
        dev = lg.device
        users, items = self._id_tensor(users, dev), self._id_tensor(items, dev)
        if lg.n == 0:
            users = users if users is not None else torch.empty(0, dtype=torch.int64, device=dev)
            m = users.numel()
            return (users, torch.full((m, k), -1, dtype=torch.int32, device=dev),
                    torch.zeros((m, k), dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev))
        eng, off, h_item, n_users, n_log_items = self._history(lg)
        lens_all = off[1:] - off[:-1]
        if users is None:
            users = torch.nonzero(lens_all > 0).flatten()
        known = users < n_users
        uc = torch.where(known, users, torch.zeros_like(users))
        lens = torch.where(known, lens_all[uc], torch.zeros_like(uc))
        l_off = torch.zeros(users.numel() + 1, dtype=torch.int64, device=dev)
        l_off[1:] = torch.cumsum(lens, 0)
        nnz = int(l_off[-1].item()) if users.numel() else 0
        within = torch.arange(nnz, dtype=torch.int64, device=dev) - torch.repeat_interleave(l_off[:-1], lens)
        l_col = h_item[torch.repeat_interleave(off[uc], lens) + within].contiguous()
        l_val = torch.ones(nnz, dtype=torch.float64, device=dev)
        n_mid = max(n_cols, n_log_items)
        mask = self._item_mask(items, n_cols, dev)
        seen = (l_off, l_col) if filter_seen_items else None
        ids, vals, count = eng.topk(eng.N.NEIGHBOUR_PREDICT, (l_off, l_col, l_val), self._csr(n_mid)[0], n_mid, n_cols, int(k),
                                    self.max_tuples, mask=mask, seen=seen)
        self.expansion = eng.expansion
        return users, ids, vals, count

    def _predict_pairs(self, pairs: pd.DataFrame, log=None, user_features=None, item_features=None) -> pd.DataFrame:
        n_rows = self._n_rows()
        if log is None:
            raise ValueError("log is not provided, but it is required for prediction")
        lg = open_log(normalise(log), str(self))
        if lg.n == 0 or len(pairs) == 0:
            return pd.DataFrame({"user_idx": np.empty(0, np.int32), "item_idx": np.empty(0, np.int32),
                                 "relevance": np.empty(0, np.float64)})
        eng, off, h_item, n_users, _ = self._history(lg)
        pu = torch.as_tensor(pairs["user_idx"].to_numpy().astype(np.int32), device=lg.device)
        pi = torch.as_tensor(pairs["item_idx"].to_numpy().astype(np.int32), device=lg.device)
        score, present = eng.pair_scores(pu, pi, off, h_item, n_users, self._csr(n_rows)[1], n_rows)
        keep = present.bool().cpu().numpy()
        return pd.DataFrame({"user_idx": pairs["user_idx"].to_numpy()[keep].astype(np.int32),
                             "item_idx": pairs["item_idx"].to_numpy()[keep].astype(np.int32),
                             "relevance": score.cpu().numpy()[keep]})

    # -------------------------------------------------------------------------------- item to item
    def get_nearest_items(self, items, k: int, metric: Optional[str] = None, candidates=None):
        """The k most similar items of each of `items` among `candidates` (None: every item); `metric` is ignored.
        Columns [item_idx, neighbour_item_idx, similarity] (base_rec.py:1554-1609)."""
        if metric is not None:
            self.logger.debug("Metric is not used to determine nearest items in %s model", str(self))
        return self._get_nearest_items_wrap(items=items, k=k, metric=None, candidates=candidates)

    def _get_nearest_items(self, items: pd.DataFrame, metric: Optional[str] = None,
                           candidates: Optional[pd.DataFrame] = None) -> pd.DataFrame:
        sim = self.similarity
        sim = sim[sim["item_idx_one"].isin(items["item_idx"])]
        if candidates is not None:
            sim = sim[sim["item_idx_two"].isin(candidates["item_idx"])]
        return sim[["item_idx_one", "item_idx_two", metric or "similarity"]]


class ItemKNN(NeighbourRec):
    """Item-based k nearest neighbours with a shrunk cosine similarity (replay/models/knn.py)."""

    bm25_k1 = 1.2
    bm25_b = 0.75
    _search_space = {
        "num_neighbours": {"type": "int", "args": [1, 100]},
        "shrink": {"type": "int", "args": [0, 100]},
        "weighting": {"type": "categorical", "args": [None, "tf_idf", "bm25"]},
    }

    def __init__(self, num_neighbours: int = 10, use_relevance: bool = False, shrink: float = 0.0,
                 weighting: Optional[str] = None, *, max_tuples: int = DEFAULT_MAX_TUPLES):
        """num_neighbours: neighbours kept per item; use_relevance: the relevance as the weight of a row instead of 1;
        shrink: added to the denominator; weighting: None, 'tf_idf' or 'bm25'; max_tuples: the tuples of the sparse
        product held in memory at once (88 bytes each) -- it does not change the result."""
        self.shrink = shrink
        self.use_relevance = use_relevance
        self.num_neighbours = num_neighbours
        valid_weightings = self._search_space["weighting"]["args"]
        if weighting not in valid_weightings:
            raise ValueError(f"weighting must be one of {valid_weightings}")
        self.weighting = weighting
        self.max_tuples = int(max_tuples)

    @property
    def _init_args(self):
        return {"shrink": self.shrink, "use_relevance": self.use_relevance, "num_neighbours": self.num_neighbours,
                "weighting": self.weighting}

    def _fit_device(self, lg) -> None:
        if self.weighting not in self._search_space["weighting"]["args"]:
            raise ValueError("weighting must be one of ['tf_idf', 'bm25']")
        N = Neigh(lg.device)
        k = int(self.num_neighbours)
        if not 1 <= k <= N.N.NEIGHBOUR_MAX_K:
            raise ValueError(f"num_neighbours must be in 1..{N.N.NEIGHBOUR_MAX_K}, got {self.num_neighbours}")
        (user, n_users), (item, n_items) = dense_ids(lg, ["user_idx", "item_idx"])
        rel = None
        if self.use_relevance:
            rel = float_column(lg, "relevance")
            if bool(torch.isnan(rel).any()):
                raise ValueError("relevance contains NaN")
        ucount, icount = N.count(user, n_users), N.count(item, n_items)
        distinct = int((icount > 0).sum().item())
        w = N.weights(user, item, rel, ucount, icount, distinct, self.weighting, self.bm25_k1, self.bm25_b)
        L, perm_i = N.view(item, n_items, user, w)
        R, _ = N.view(user, n_users, item, w)
        norm = N.norms(perm_i, L[0], w, n_items)
        self._clear_cache()
        ids, vals, count = N.topk(N.N.NEIGHBOUR_FIT, L, R, n_users, n_items, k, self.max_tuples, norm_q=norm, norm_j=norm,
                                  shrink=float(self.shrink))
        self._sim = Padded(ids, {"similarity": vals}, count)
        self.row_weights, self.item_norms, self.expansion = w, norm, N.expansion
