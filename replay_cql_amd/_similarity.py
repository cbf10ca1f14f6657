"""The two formats of a fitted item-to-item similarity table, as `NeighbourRec` holds one in `_sim` and returns it from
`similarity_device`.  Both are tuples of device tensors with three things on top, all `NeighbourRec` asks of a table:
`n_rows`, `frame()` and `csr(n_rows, plane)`."""
from __future__ import annotations

from typing import Dict, NamedTuple

import numpy as np
import pandas as pd
import torch

from .device_recommender import DeviceRecommender

_first = DeviceRecommender._first          # bool mask [n, k]: the first counts[r] slots of row r


class Padded(tuple):
    """(ids int32 [n_items, K] padded with -1, one float64 [n_items, K] plane per measure, counts int32 [n_items]): row i
    holds the neighbours of item i, best first.  ItemKNN has the one plane `similarity`; the association rules have
    `confidence`, `lift` and `confidence_gain`."""

    def __new__(cls, ids, planes: Dict[str, torch.Tensor], counts):
        self = super().__new__(cls, (ids, *planes.values(), counts))
        self.names = tuple(planes)
        return self

    def plane(self, name: str):
        return self[1 + self.names.index(name)]

    @property
    def n_rows(self) -> int:
        """one row per item id below the largest fitted one + 1"""
        return int(self[0].shape[0])

    def frame(self) -> pd.DataFrame:
        """[item_idx_one, item_idx_two, one column per plane], by item_idx_one ascending, then rank"""
        ids, counts = self[0], self[-1]
        keep = _first(ids, counts).cpu().numpy()
        one = np.broadcast_to(np.arange(ids.shape[0], dtype=np.int32)[:, None], keep.shape)[keep]
        return pd.DataFrame({"item_idx_one": one, "item_idx_two": ids.cpu().numpy()[keep],
                             **{name: self.plane(name).cpu().numpy()[keep] for name in self.names}})

    def csr(self, n_rows: int, plane: str):
        """the plane as CSR with n_rows >= n_items rows: (offsets, columns, values) in rank order, and sorted by column"""
        ids, vals, counts = self[0], self.plane(plane), self[-1]
        off = torch.zeros(n_rows + 1, dtype=torch.int64, device=ids.device)
        off[1:ids.shape[0] + 1] = torch.cumsum(counts.to(torch.int64), 0)
        off[ids.shape[0] + 1:] = off[ids.shape[0]]
        keep = _first(ids, counts)
        col, val = ids[keep].contiguous(), vals[keep].contiguous()
        row = torch.arange(ids.shape[0], device=ids.device, dtype=torch.int64)[:, None].expand_as(ids)[keep]
        by_col = torch.argsort(row * max(1, ids.shape[0]) + col.to(torch.int64))
        return (off, col, val), (off, col[by_col].contiguous(), val[by_col].contiguous())


class Csr(NamedTuple):
    """(offsets int64 [n_items + 1], item_idx_two int32 ascending inside a row, similarity float64): row i holds the
    non-zeros of row i of a fitted n_items x n_items matrix (ADMMSLIM, SLIM), where a row can be n_items wide"""
    offsets: torch.Tensor
    columns: torch.Tensor
    values: torch.Tensor

    @property
    def n_rows(self) -> int:
        return int(self.offsets.numel()) - 1

    def frame(self) -> pd.DataFrame:
        """[item_idx_one, item_idx_two, similarity]: the non-zeros of the fitted matrix, row-major"""
        lens = (self.offsets[1:] - self.offsets[:-1]).cpu().numpy()
        return pd.DataFrame({"item_idx_one": np.repeat(np.arange(len(lens), dtype=np.int32), lens),
                             "item_idx_two": self.columns.cpu().numpy(), "similarity": self.values.cpu().numpy()})

    def csr(self, n_rows: int, plane: str = "similarity"):
        """the table with n_rows >= n_items rows; the columns of a row ascend, so one CSR serves both readers"""
        off = self.offsets
        if n_rows + 1 > off.numel():
            off = torch.cat([off, off[-1:].expand(n_rows + 1 - off.numel())])
        return (off, self.columns, self.values), (off, self.columns, self.values)
