"""The Indexer of replay/data_preparator.py on the GPU, for integer raw ids: `fit(users, items)`, `transform(df)`,
`inverse_transform(df)` and `_init_args` as the reference has them.  Everything downstream -- the splitters' count
arrays and bitmaps, E_in / E_out -- needs dense user_idx / item_idx, and a filter leaves holes: this closes them on the
device (csrc/prepare.hip: radix sort + unique for the labels, a binary search per row for the lookup, a gather back).

Frames are what the splitters take (pandas, a pyarrow Table / RecordBatch / sequence of batches, a dict of device
tensors) and come back as the kind given, rows in input order.  Importing this module and constructing an Indexer needs
no GPU; fit / transform / inverse_transform do (CqlrecError without one).

Where this deviates from the reference, on purpose:
  * integer ids only.  Any int64 value is a legal raw id, negative and sparse ones included.  A string or float id
    column raises ValueError: factorize it on the host first (pandas.factorize) -- strings have no place on the device;
  * label order.  fit's labels are the distinct ids in ASCENDING NUMERIC order; Spark's StringIndexer orders them by
    frequency and then by the id's string form.  `user_labels` / `item_labels` (int64 device tensors) are public:
    label[idx] is the raw id of index idx;
  * ids that fit did not see are appended by transform behind the existing labels, in ascending id order (the
    reference's _reindex appends them in the order a Python set yields them); existing indices never move.

transform replaces item_col by int32 item_idx and user_col by int32 user_idx; the column order follows the reference:
user_idx, item_idx, then the rest (or just the one id column that is present).  inverse_transform maps user_idx /
item_idx back to the original column names and the integer dtype the columns had at fit; an index outside the labels
raises ValueError."""
from __future__ import annotations

import numpy as np
import torch

from . import _log as L
from . import _prepare as P

__all__ = ["Indexer"]


def _np_dtype(dt) -> np.dtype:
    return np.dtype(str(dt).replace("torch.", "")) if isinstance(dt, torch.dtype) else np.dtype(dt)


def _raw_id_dtype(frame, name: str) -> np.dtype:
    kind, dt = L.column_kind(frame, name)
    if kind not in "iu":
        raise ValueError(f"column {name} must hold integer ids (it is {'float' if kind == 'f' else 'no number'}): "
                         "factorize other ids on the host first, e.g. pandas.factorize")
    dt = _np_dtype(dt)
    if dt == np.uint64:
        raise ValueError(f"column {name}: uint64 ids do not fit the int64 labels")
    return dt


def _assemble(lg, drop, front):
    """The frame of `lg` without the columns `drop`, the columns `front` ({name: (device tensor, numpy dtype)}) first."""
    rest = [nm for nm in lg.names if nm not in drop]
    if lg.kind == "device":
        out = {nm: t.to(getattr(torch, dt.name)) for nm, (t, dt) in front.items()}
        out.update((nm, lg.src[nm]) for nm in rest)
        return out
    host = {nm: t.cpu().numpy().astype(dt, copy=False) for nm, (t, dt) in front.items()}
    if lg.kind == "pandas":
        out = lg.src[rest].reset_index(drop=True)
        for pos, (nm, a) in enumerate(host.items()):
            out.insert(pos, nm, a)
        return out
    import pyarrow as pa
    names = list(host) + rest
    arrays = [pa.array(a) for a in host.values()] + [lg.table.column(nm) for nm in rest]
    if lg.kind == "batch":
        arrays = [a.combine_chunks() if isinstance(a, pa.ChunkedArray) else a for a in arrays]
        return pa.RecordBatch.from_arrays(arrays, names=names)
    return pa.Table.from_arrays(arrays, names=names)


class Indexer:
    """Converts raw integer ids to dense indices and back."""

    def __init__(self, user_col="user_id", item_col="item_id"):
        self.user_col = user_col
        self.item_col = item_col
        self.user_type = self.item_type = None              # numpy dtypes of the raw id columns, set by fit
        self.user_labels = self.item_labels = None          # int64 device tensors, set by fit: label[idx] = raw id
        self._sorted = {}                                   # entity -> (labels the pair was made from, sorted, index)

    @property
    def _init_args(self):
        return {"user_col": self.user_col, "item_col": self.item_col}

    # ---- labels ---------------------------------------------------------------------------------------------
    def _labels(self, entity: str):
        labels = getattr(self, f"{entity}_labels")
        if labels is None:
            raise ValueError("the Indexer is not fitted: call fit(users, items) first")
        return labels

    def _search_arrays(self, entity: str, prep):
        labels = self._labels(entity)
        cached = self._sorted.get(entity)
        if cached is None or cached[0] is not labels:
            cached = (labels,) + prep.sort_labels(labels)
            self._sorted[entity] = cached
        return cached[1], cached[2]

    @staticmethod
    def _distinct(src, col: str):
        lg = L.open_log(src, "Indexer.fit")
        if lg.n == 0:
            return torch.empty(0, dtype=torch.int64, device=lg.device)
        return P.Prep(lg.device).distinct(lg.ids(col))

    def fit(self, users, items) -> None:
        """Labels of the distinct ids of `users[user_col]` and `items[item_col]`, in ascending numeric order."""
        users, items = L.normalise(users), L.normalise(items)
        user_type, item_type = _raw_id_dtype(users, self.user_col), _raw_id_dtype(items, self.item_col)
        user_labels, item_labels = self._distinct(users, self.user_col), self._distinct(items, self.item_col)
        self.user_labels, self.user_type, self.item_labels, self.item_type = user_labels, user_type, item_labels, item_type
        self._sorted = {}

    def _index(self, entity: str, ids, prep):
        """int32 indices of the raw ids; ids not among the labels are appended to them first, ascending"""
        idx, miss = prep.lookup(ids, *self._search_arrays(entity, prep))
        if miss:
            new = prep.distinct(ids[idx < 0])
            labels = torch.cat([self._labels(entity), new])
            if labels.numel() >= (1 << 31) - 1:
                raise ValueError("more than 2^31 - 2 labels")
            setattr(self, f"{entity}_labels", labels)
            idx, miss = prep.lookup(ids, *self._search_arrays(entity, prep))
            assert not miss
        return idx

    # ---- frames ---------------------------------------------------------------------------------------------
    def transform(self, df):
        """Raw `user_col` / `item_col` -> int32 `user_idx` / `item_idx`, in front of the other columns."""
        src = L.normalise(df)
        present = []
        for entity, col in (("item", self.item_col), ("user", self.user_col)):      # the reference's order
            if not L.has_column(src, col):
                continue
            _raw_id_dtype(src, col)
            self._labels(entity)
            present.append((entity, col))
        lg = L.open_log(src, "Indexer.transform")
        prep = P.Prep(lg.device)
        done = {}
        for entity, col in present:
            idx = torch.empty(0, dtype=torch.int32, device=lg.device) if lg.n == 0 else \
                self._index(entity, lg.ids(col), prep)
            done[entity] = (idx, np.dtype(np.int32))
        front = {f"{e}_idx": done[e] for e in ("user", "item") if e in done}
        return _assemble(lg, {col for _, col in present}, front)

    def inverse_transform(self, df):
        """`user_idx` / `item_idx` -> the raw ids under their original column names and dtype."""
        src = L.normalise(df)
        present = []
        for entity in ("item", "user"):
            if not L.has_column(src, f"{entity}_idx"):
                continue
            if L.column_kind(src, f"{entity}_idx")[0] not in "iu":
                raise ValueError(f"column {entity}_idx must be an integer column")
            self._labels(entity)
            present.append(entity)
        lg = L.open_log(src, "Indexer.inverse_transform")
        prep = P.Prep(lg.device)
        done = {}
        for entity in present:
            dt = getattr(self, f"{entity}_type")
            if lg.n == 0:
                raw = torch.empty(0, dtype=torch.int64, device=lg.device)
            else:
                raw, bad = prep.gather(lg.ids(f"{entity}_idx"), self._labels(entity))
                if bad:
                    raise ValueError(f"{entity}_idx holds an index outside the {self._labels(entity).numel()} labels")
            done[entity] = (raw, dt)
        front = {getattr(self, f"{e}_col"): done[e] for e in ("user", "item") if e in done}
        return _assemble(lg, {f"{e}_idx" for e in present}, front)
