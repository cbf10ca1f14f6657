"""`DeviceRecommender`: what the models fitted and scored on the device share (`ALSWrap`, `NeighbourRec` / `ItemKNN`) on
top of the pandas template of recommender_api.py, which stays free of torch.

A subclass names the attribute its fitted state lives in (`_state_attr`) and implements `_fit_device(lg)`,
`_recommend(log, k, users, items, filter_seen_items)` and `_predict_pairs`.  `_recommend` returns at most k rows per
user, already without the seen items when `filter_seen_items` is set, so the template's `_filter_seen` and
`get_top_k_recs` change nothing after `_predict`."""
from __future__ import annotations

from abc import abstractmethod
from typing import Dict, Optional

import numpy as np
import pandas as pd
import torch

from . import _log as L
from .recommender_api import REC_COLUMNS, PandasRecommender


class DeviceRecommender(PandasRecommender):
    _state_attr: str

    # -------------------------------------------------------------------------------- fit
    def _fit_wrap(self, log, user_features=None, item_features=None) -> None:
        """pandas and Spark logs go through the template; a pyarrow log or a dict of device tensors stays on the device"""
        src = L.normalise(log)
        if isinstance(src, pd.DataFrame) or type(src).__module__.startswith("pyspark"):
            super()._fit_wrap(src, user_features, item_features)
            return
        lg = L.open_log(src, str(self))
        if lg.n == 0:
            raise ValueError("cannot fit an empty log")
        users, items = torch.unique(lg.ids("user_idx")).cpu().numpy(), torch.unique(lg.ids("item_idx")).cpu().numpy()
        self.fit_users, self.fit_items = pd.DataFrame({"user_idx": users}), pd.DataFrame({"item_idx": items})
        self._num_users, self._num_items = len(users), len(items)
        self._user_dim_size, self._item_dim_size = int(users.max()) + 1, int(items.max()) + 1
        self._fit_device(lg)

    def _fit(self, log: pd.DataFrame, user_features=None, item_features=None) -> None:
        self._fit_device(L.open_log(log, str(self)))

    @abstractmethod
    def _fit_device(self, lg) -> None:
        ...

    def _fitted(self):
        if self._state_attr not in self.__dict__:
            raise RuntimeError(f"{self} model is not fitted")
        return self.__dict__[self._state_attr]

    # -------------------------------------------------------------------------------- predict on the device
    @staticmethod
    def _id_tensor(ids, device) -> Optional[torch.Tensor]:
        """distinct non-negative ids as an int64 device tensor, in the order given"""
        if ids is None:
            return None
        if torch.is_tensor(ids):
            t = ids.to(device=device, dtype=torch.int64).flatten()
        else:
            if isinstance(ids, pd.DataFrame):
                ids = ids.iloc[:, 0]
            t = torch.as_tensor(np.asarray(pd.unique(pd.Series(ids)), dtype=np.int64), device=device)
        return t[t >= 0]

    @staticmethod
    def _item_mask(items, n_items: int, device):
        """uint8 [n_items], 1 at the ids of `items` below n_items; None for None (every item)"""
        if items is None:
            return None
        mask = torch.zeros(n_items, dtype=torch.uint8, device=device)
        mask[items[items < n_items]] = 1
        return mask

    @staticmethod
    def _first(ids, count):
        """bool mask of the shape of `ids` [n, k]: the first count[r] slots of row r"""
        return torch.arange(ids.shape[1], device=ids.device)[None, :] < count[:, None]

    @abstractmethod
    def _recommend(self, log, k: int, users, items, filter_seen_items: bool):
        """(users int64 [m], ids int32 [m, k], values [m, k], count int32 [m]) on the device"""

    def recommend(self, log, k: int, users=None, items=None, filter_seen_items: bool = True) -> Dict[str, torch.Tensor]:
        """The k best items of every user as device columns {user_idx int32, item_idx int32, relevance float64}, in the
        order of `users` (None: the users of the log, ascending), then rank.  `log`: pandas, pyarrow or a dict of device
        tensors; a model that needs no log to score (ALSWrap) also takes None: nothing is seen then, and users=None is every
        user that has a factor.  `users` / `items`: tensors, iterables or None (every item).  Ids the model cannot score
        (no factor, no similarity row) are absent."""
        users, ids, vals, count = self._recommend(log, int(k), users, items, filter_seen_items)
        keep = self._first(ids, count)
        return {"user_idx": users.to(torch.int32)[:, None].expand_as(ids)[keep], "item_idx": ids[keep],
                "relevance": vals[keep].to(torch.float64)}

    def _predict(self, log, k: int, users: pd.DataFrame, items: pd.DataFrame, user_features=None, item_features=None,
                 filter_seen_items: bool = True) -> pd.DataFrame:
        out = self.recommend(log, k, users["user_idx"], items["item_idx"], filter_seen_items)
        return pd.DataFrame({c: out[c].cpu().numpy() for c in REC_COLUMNS})
