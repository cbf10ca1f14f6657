"""Association rules on the device: `AssociationRulesItemRec` (replay/models/association_rules.py) over the rules
epilogue of csrc/neighbour.hip (section f10 of include/cqlrec.h).  DESIGN.md section 3.13 is the normative text.

`fit` is the engine of `NeighbourRec` -- the row-wise top-k of a sparse x sparse product, items x sessions times
sessions x items -- with min(w_a, w_b) in place of the product, a pair count as the filter, and three measures per kept
pair: confidence, lift and confidence gain.  The rows of the log are made distinct first ((session, item, weight)
triples), then the items below `min_item_count` leave.  `predict`, `predict_pairs`, `recommend` and `get_nearest_items`
are `NeighbourRec`'s, reading the value plane that `similarity_metric` names; the metric may change after `fit`.

Deviations from the reference, both stated in DESIGN.md section 3.13: a pair whose antecedent or consequent relevance
sums to 0 is dropped (the reference divides by zero), and `num_neighbours=None` keeps all pairs only up to
NEIGHBOUR_MAX_K + 1 items (k = n_items - 1 must fit the engine's limit; beyond it `fit` raises).

Nothing here has a CPU path: without a GPU every call that computes raises CqlrecError."""
from __future__ import annotations

from typing import List, Optional

import pandas as pd
import torch

from ._log import dense_ids, float_column
from ._similarity import Padded
from .neighbour import DEFAULT_MAX_TUPLES, Neigh, NeighbourRec

__all__ = ["AssociationRulesItemRec"]


class AssociationRulesItemRec(NeighbourRec):
    """Item-to-item recommender on association rules: per antecedent item the `num_neighbours` consequents of the largest
    lift, each with its confidence, lift and confidence gain = confidence(a, b) / confidence(!a, b)."""

    can_predict_item_to_item = True
    can_change_metric = True
    item_to_item_metrics: List[str] = ["lift", "confidence", "confidence_gain"]
    _search_space = {
        "min_item_count": {"type": "int", "args": [3, 10]},
        "min_pair_count": {"type": "int", "args": [3, 10]},
        "num_neighbours": {"type": "int", "args": [300, 2000]},
        "use_relevance": {"type": "categorical", "args": [True, False]},
        "similarity_metric": {"type": "categorical", "args": ["confidence", "lift"]},
    }

    # pylint: disable=too-many-arguments
    def __init__(self, session_col: Optional[str] = None, min_item_count: int = 5, min_pair_count: int = 5,
                 num_neighbours: Optional[int] = 1000, use_relevance: bool = False, similarity_metric: str = "confidence",
                 *, max_tuples: int = DEFAULT_MAX_TUPLES):
        """session_col: the column that groups rows into sessions (None: user_idx); min_item_count: items with fewer
        distinct rows leave; min_pair_count: pairs that co-occur less often leave; num_neighbours: pairs kept per
        antecedent (None: all, for at most NEIGHBOUR_MAX_K + 1 items); use_relevance: the relevance as the weight of a
        row instead of 1 -- a pair then weighs the smaller of its two; similarity_metric: the measure predict sums;
        max_tuples: the tuples of the sparse product held in memory at once (88 bytes each) -- it does not change the
        result."""
        self.session_col = session_col if session_col is not None else "user_idx"
        self.min_item_count = min_item_count
        self.min_pair_count = min_pair_count
        self.num_neighbours = num_neighbours
        self.use_relevance = use_relevance
        self.similarity_metric = similarity_metric
        self.max_tuples = int(max_tuples)

    @property
    def _init_args(self):
        return {"session_col": self.session_col, "min_item_count": self.min_item_count,
                "min_pair_count": self.min_pair_count, "num_neighbours": self.num_neighbours,
                "use_relevance": self.use_relevance, "similarity_metric": self.similarity_metric}

    # -------------------------------------------------------------------------------- fit
    def _fit_device(self, lg) -> None:
        N = Neigh(lg.device)
        limit = N.N.NEIGHBOUR_MAX_K
        (session, n_sessions), (item, n_items) = dense_ids(lg, [self.session_col, "item_idx"])
        if self.num_neighbours is None:
            k = max(1, n_items - 1)
            if k > limit:
                raise ValueError(f"num_neighbours=None keeps n_items - 1 = {k} pairs per item, beyond the limit of {limit}: "
                                 f"give num_neighbours in 1..{limit}")
        else:
            k = int(self.num_neighbours)
            if not 1 <= k <= limit:
                raise ValueError(f"num_neighbours must be in 1..{limit}, got {self.num_neighbours}")
        rel = None
        if self.use_relevance:
            rel = float_column(lg, "relevance")
            if not bool(torch.isfinite(rel).all()):
                raise ValueError("relevance contains NaN or an infinite value")
        # the distinct (session, item, weight) rows: order by (session, item, weight), mark, compact
        perm, _ = N.segments(item, n_items, None if rel is None else (rel + 0.0).view(torch.int64))
        by_session, _ = N.segments(session[perm.long()].contiguous(), n_sessions)
        perm = perm[by_session.long()].contiguous()
        rows = N.compact(N.rules_distinct(session, item, rel, perm))
        session, item = session[rows].contiguous(), item[rows].contiguous()
        w = rel[rows].contiguous() if rel is not None else torch.ones(rows.numel(), dtype=torch.float64, device=lg.device)
        num_sessions = int((N.count(session, n_sessions) > 0).sum().item())
        # the item filter, then the two views of what is left
        item_count = N.count(item, n_items)
        rows = N.compact((item_count[item.long()] >= int(self.min_item_count)).to(torch.uint8))
        session, item, w = session[rows].contiguous(), item[rows].contiguous(), w[rows].contiguous()
        if rows.numel():
            L, _ = N.view(item, n_items, session, w)
            R, _ = N.view(session, n_sessions, item, w)
        else:                                                                # no row left: an empty product
            L = (torch.zeros(n_items + 1, dtype=torch.int64, device=lg.device), session, w)
            R = (torch.zeros(n_sessions + 1, dtype=torch.int64, device=lg.device), item, w)
        self._clear_cache()
        ids, conf, lift, gain, count, item_rel = N.rules_topk(L, R, n_sessions, k, self.max_tuples, num_sessions,
                                                              int(self.min_pair_count))
        # row a holds the consequents of item a, largest lift first
        self._sim = Padded(ids, {"confidence": conf, "lift": lift, "confidence_gain": gain}, count)
        self.num_sessions, self.item_count, self.item_relevance = num_sessions, item_count, item_rel
        self.expansion, self.row_prefix = N.expansion, N.row_prefix        # the host row prefix: where the chunks were cut

    # -------------------------------------------------------------------------------- the table
    @property
    def get_similarity(self) -> pd.DataFrame:
        """the measures calculated during `fit`"""
        return self.similarity

    # -------------------------------------------------------------------------------- item to item
    def get_nearest_items(self, items, k: int, metric: str = "lift", candidates=None):
        """The k consequents of each of `items` with the largest `metric`, among `candidates` (None: every item).
        Columns [item_idx, neighbour_item_idx, <metric>]."""
        if metric not in self.item_to_item_metrics:
            raise ValueError(f"Select one of the valid distance metrics: {self.item_to_item_metrics}")
        return self._get_nearest_items_wrap(items=items, k=k, metric=metric, candidates=candidates)
