"""The feature processors of replay/history_based_fp.py on the GPU: EmptyFeatureProcessor, LogStatFeaturesProcessor,
ConditionalPopularityProcessor and HistoryBasedFeaturesProcessor, with the reference's constructor, fit and transform
signatures, the `fitted` attribute and AttributeError("Call fit before running transform").  What the reference does
with a dozen Spark group-bys and two left joins is sorted segments, fixed-order fp64 sums, binary searches and one
fused gather here -- csrc/features.hip (section f7 of include/cqlrec.h), deterministic: the same log gives the same
bytes.

A log or a frame of pairs is what the filters take -- a pandas DataFrame, a pyarrow Table / RecordBatch / sequence of
batches, or a dict of device tensors; `transform(frame)` returns the kind it was given, every column carried, rows in
input order, the feature columns appended under the reference's names.  `user_idx` / `item_idx` are dense non-negative
integer ids, range-checked before any launch at fit.  Importing this module needs no GPU; calling without one raises
CqlrecError.  An empty log fits to empty tables without a launch.

Fitted tables are dense device tensors indexed by id; an id without rows has count 0 and is "cold".
`user_log_features` / `item_log_features` are also offered as pandas frames of the present ids in ascending order.

`transform_block(user_idx, item_idx, dtype=torch.float32)` returns `(block, names)`: a row-major [n_pairs, F] device
tensor written by ONE kernel, and the names of its columns, in this order:
  1. the numeric columns of the user table, then of the item table, each in the order of its frame (the four
     `*_interact_date` columns are left out: `*_history_length_days` and `*_last_interaction_gap_days` carry them);
  2. na_u_log_features, na_i_log_features;
  3. u_i_log_num_interact_diff, i_u_log_num_interact_diff;
  4. for every conditional-popularity column, user features first: <e>_pop_by_<col>, na_<e>_pop_by_<col> (1.0 / 0.0).
`transform` builds its feature columns from the float64 block of the same kernel.

Semantics, and where they deviate from the reference on purpose:
  * calc_relevance_based: relevance has more than one distinct value; a NaN relevance raises ValueError.
    calc_timestamp_based: the timestamp column is a datetime or an integer (unix seconds) with more than one distinct
    value.  A float (or missing) timestamp column gives no time features (the reference requires TimestampType).
  * a day is floor(t / 86 400 s) (floor division; the reference truncates in the session time zone's calendar).
  * std is the sample standard deviation (n - 1), 0 for a group of one row; it is computed in two passes.
  * quantile_05 / _5 / _95 are the elements of the group's ascending relevances at the 1-based rank
    clamp(ceil(p * n), 1, n), p * n one IEEE double multiply: Spark's percentile_approx while that is exact (roughly
    below 10 000 rows per group).  DEVIATION: exact at every size.
  * abnormalityCR exists iff max(i_std) - min(i_std) != 0 over the present items, as in the reference.
  * transform is a left join: na_u_log_features / na_i_log_features are 1.0 for a cold id or an id beyond the table,
    every joined numeric column is 0 there, date columns are NaT / null (the int64 minimum in a dict of tensors); the
    two *_log_num_interact_diff columns are computed after the fill.
  * ConditionalPopularityProcessor: `features` holds item_idx or user_idx plus the categorical columns; the OTHER
    entity receives the features.  Categories of any dtype are factorized on the host at fit; an id missing from
    `features` and a null / NaN category form the null category (the left join).  At transform the category comes from
    the frame's column when it has one, otherwise from the table fitted per id; an unseen value is `na`, and so is the
    null category (a join never matches null to null, as in Spark).  DEVIATION: when `features` lists an id twice the
    last row counts (the reference's join would duplicate the log rows).
  * DEVIATION: HistoryBasedFeaturesProcessor builds the item-side processor whenever item_cat_features_list is given
    (the reference only when the user list is given too)."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import _log as L
from . import _prepare as P

__all__ = ["EmptyFeatureProcessor", "LogStatFeaturesProcessor", "ConditionalPopularityProcessor",
           "HistoryBasedFeaturesProcessor"]

DAY_S = 86400
_NAT = L.I64_MIN                                   # numpy's NaT bit pattern
_STAT_COLS = ("std", "mean", "quantile_05", "quantile_5", "quantile_95")     # the reference's order; table: 2 1 3 4 5
_STAT_AT = (2, 1, 3, 4, 5)
_INT_COLS = ("history_length_days", "last_interaction_gap_days")


def _id_column(log, name) -> None:
    kind, _ = L.column_kind(log, name)
    if kind not in "iu":
        raise ValueError(f"column {name} must be an integer column")


def _pair_ids(lg):
    return lg.ids("user_idx"), lg.ids("item_idx")


def _append(lg, cols: Dict[str, object], datetime_dates: bool):
    """The frame `lg` was made of with the columns `cols` (name -> device tensor) appended, as the kind that came in.
    A `*_interact_date` column holds int64 keys, the int64 minimum where the id is cold: NaT / null on the host."""
    if lg.kind == "device":
        out = dict(lg.src)
        out.update(cols)
        return out
    host = {k: v.cpu().numpy() for k, v in cols.items()}
    dates = [k for k in host if k.endswith("_interact_date")]
    if lg.kind == "pandas":
        import pandas as pd
        out = lg.src.copy()
        for k, v in host.items():
            if k in dates:
                v = v.view("datetime64[ns]") if datetime_dates else pd.arrays.IntegerArray(v, v == _NAT)
            out[k] = v
        return out
    import pyarrow as pa
    tab = lg.table
    for k, v in host.items():
        if k in tab.schema.names:
            tab = tab.drop([k])
        if k in dates:
            col = pa.array(v.view("datetime64[ns]") if datetime_dates else v, mask=v == _NAT)
        else:
            col = pa.array(v)
        tab = tab.append_column(k, col)
    if lg.kind == "batch":
        tab = tab.combine_chunks()
        return tab.to_batches()[0] if tab.num_rows else pa.RecordBatch.from_pylist([], schema=tab.schema)
    return tab


class EmptyFeatureProcessor:
    """Do not perform any transformations on the frame."""

    def fit(self, log, features=None) -> None:
        """:param log: ``[user_idx, item_idx, timestamp, relevance]``;  :param features: ids and feature columns"""

    def transform(self, log):
        return log


class LogStatFeaturesProcessor(EmptyFeatureProcessor):
    """User and item features from the interaction log: log counts, their cross means, day counts and spans, relevance
    mean / std / quantiles, abnormality (see the module docstring)."""

    calc_timestamp_based: bool = False
    calc_relevance_based: bool = False

    def __init__(self):
        self._fit_done = False

    # ---- fit ---------------------------------------------------------------------------------------------------
    def fit(self, log, features=None) -> None:
        src = L.normalise(log)
        for name in ("user_idx", "item_idx"):
            _id_column(src, name)
        rel_kind, _ = L.column_kind(src, "relevance")
        if rel_kind not in "iufb":
            raise ValueError("column relevance must be a numeric column")
        ts_kind = L.column_kind(src, "timestamp")[0] if L.has_column(src, "timestamp") else None
        lg = L.open_log(src, "LogStatFeaturesProcessor.fit")
        self.calc_timestamp_based = self.calc_relevance_based = self._has_cr = False
        self._ts_kind, self._dev = None, lg.device
        self._n_users = self._n_items = 0
        self._udates = self._idates = self._udays = self._idays = None
        if lg.n == 0:
            self._ucount = self._icount = torch.zeros(0, dtype=torch.int32, device=lg.device)
            self._set_tables({"u_log_num_interact": None, "u_mean_i_log_num_interact": None},
                             {"i_log_num_interact": None, "i_mean_u_log_num_interact": None})
            return
        (user, n_users), (item, n_items) = L.dense_ids(lg, ["user_idx", "item_idx"])
        self._n_users, self._n_items = n_users, n_items
        feat = P.Feat(lg.device)
        rel = L.float_column(lg, "relevance")
        lim = torch.stack([rel.min(), rel.max()]).cpu().tolist()          # torch's min / max propagate NaN
        if lim[0] != lim[0] or lim[1] != lim[1]:
            raise ValueError("relevance contains NaN")
        self.calc_relevance_based = lim[0] != lim[1]
        key = None
        if ts_kind is not None and ts_kind in "Miu":
            key = lg.key("timestamp")
            glo, ghi = (int(x) for x in torch.cat(feat.minmax(None, 1, key)).cpu().tolist())
            self.calc_timestamp_based = glo != ghi
            self._ts_kind = lg.ts_kind
        sides = {}
        from .data import timestamp_key
        rel_key = timestamp_key(rel).contiguous() if self.calc_relevance_based else None
        unit = DAY_S * (10 ** 9 if self._ts_kind == "datetime" else 1)
        day = feat.day(key, unit) if self.calc_timestamp_based else None
        for pre, group, n_groups in (("u", user, n_users), ("i", item, n_items)):
            d = {"count": feat.count(group, n_groups)}
            d["perm"], d["offsets"] = feat.segments(group, n_groups, rel_key)
            cols = {f"{pre}_log_num_interact": torch.log(d["count"].to(torch.float64))}
            if self.calc_timestamp_based:
                perm_d, off_d = feat.segments(group, n_groups, day)
                days = feat.segment_distinct(group, perm_d, off_d, day, n_groups)
                lo, hi = feat.minmax(group, n_groups, key)
                d["dates"], d["days"] = (lo, hi), days
                cols[f"{pre}_log_interact_days_count"] = torch.log(days.to(torch.float64))
            if self.calc_relevance_based:
                st = feat.segment_stats(d["perm"], d["offsets"], rel, n_groups)
                d["stats"] = st
                for name, at in zip(_STAT_COLS, _STAT_AT):
                    cols[f"{pre}_{name}"] = st[:, at]
            if self.calc_timestamp_based:
                day_lo, day_hi = feat.day(lo, unit), feat.day(hi, unit)
                cols[f"{pre}_history_length_days"] = (day_hi - day_lo).to(torch.float64)
                cols[f"{pre}_last_interaction_gap_days"] = (ghi // unit - day_hi).to(torch.float64)
            d["cols"] = cols
            sides[pre] = d
        u, i = sides["u"], sides["i"]
        if self.calc_relevance_based:
            ist = i["stats"]
            u["cols"]["abnormality"] = feat.segment_mean(feat.N.FEATURES_MEAN_ABNORMALITY, u["perm"], u["offsets"], n_users,
                                                         item, ist[:, 1], value=rel)
            std_present = ist[:, 2][i["count"] > 0]
            lo_s, hi_s = torch.stack([std_present.min(), std_present.max()]).cpu().tolist()
            if hi_s - lo_s != 0:
                self._has_cr = True
                u["cols"]["abnormalityCR"] = feat.segment_mean(feat.N.FEATURES_MEAN_ABNORMALITY_CR, u["perm"], u["offsets"],
                                                               n_users, item, ist[:, 1], ist[:, 2], value=rel,
                                                               min_std=lo_s, max_std=hi_s)
        # the log counts enter the cross means as they stand in the tables: finite for every id a row names
        ilog = i["cols"]["i_log_num_interact"].contiguous()
        ulog = u["cols"]["u_log_num_interact"].contiguous()
        u["cols"]["u_mean_i_log_num_interact"] = feat.segment_mean(feat.N.FEATURES_MEAN_GATHER, u["perm"], u["offsets"],
                                                                   n_users, item, ilog)
        i["cols"]["i_mean_u_log_num_interact"] = feat.segment_mean(feat.N.FEATURES_MEAN_GATHER, i["perm"], i["offsets"],
                                                                   n_items, user, ulog)
        self._ucount, self._icount = u["count"], i["count"]
        self._udates, self._idates = u.get("dates"), i.get("dates")
        self._udays, self._idays = u.get("days"), i.get("days")          # distinct days per id, int32
        self._set_tables(u["cols"], i["cols"])

    def _set_tables(self, ucols, icols) -> None:
        def pack(cols, count, n):
            if n == 0:
                return torch.zeros((0, len(cols)), dtype=torch.float64, device=self._dev)
            cold = (count == 0).unsqueeze(1)
            return torch.where(cold, 0.0, torch.stack(list(cols.values()), dim=1)).contiguous()
        self._unames, self._inames = list(ucols), list(icols)
        self._utab = pack(ucols, self._ucount, self._n_users)
        self._itab = pack(icols, self._icount, self._n_items)
        self._fit_done = True

    # ---- fitted tables as frames --------------------------------------------------------------------------------
    def _frame(self, pre: str):
        import pandas as pd
        if not self._fit_done:
            return None
        tab, names, count, dates = ((self._utab, self._unames, self._ucount, self._udates) if pre == "u" else
                                    (self._itab, self._inames, self._icount, self._idates))
        ids = torch.nonzero(count > 0).flatten()
        host = tab[ids].cpu().numpy()
        out = {("user_idx" if pre == "u" else "item_idx"): ids.cpu().numpy()}
        for j, name in enumerate(names):
            col = host[:, j]
            out[name] = col.astype(np.int64) if name[2:] in _INT_COLS else col
            if name == f"{pre}_log_interact_days_count":
                for which, keys in zip(("min", "max"), dates):
                    out[f"{pre}_{which}_interact_date"] = self._host_dates(keys[ids].cpu().numpy())
        return pd.DataFrame(out)

    def _host_dates(self, keys: np.ndarray):
        return keys.view("datetime64[ns]") if self._ts_kind == "datetime" else keys

    @property
    def user_log_features(self):
        return self._frame("u")

    @property
    def item_log_features(self):
        return self._frame("i")

    # ---- transform ----------------------------------------------------------------------------------------------
    def _block_parts(self):
        """(colmap entries, names) of this processor's share of a block"""
        from . import _native as N
        cm = [(N.FEATURES_COL_USER, j, 0) for j in range(len(self._unames))]
        cm += [(N.FEATURES_COL_ITEM, j, 0) for j in range(len(self._inames))]
        cm += [(N.FEATURES_COL_NA_USER, 0, 0), (N.FEATURES_COL_NA_ITEM, 0, 0),
               (N.FEATURES_COL_DIFF_USER, self._unames.index("u_log_num_interact"),
                self._inames.index("i_mean_u_log_num_interact")),
               (N.FEATURES_COL_DIFF_ITEM, self._inames.index("i_log_num_interact"),
                self._unames.index("u_mean_i_log_num_interact"))]
        names = self._unames + self._inames + ["na_u_log_features", "na_i_log_features", "u_i_log_num_interact_diff",
                                               "i_u_log_num_interact_diff"]
        return cm, names

    def _frame_columns(self, block, names, user, item) -> Dict[str, object]:
        """name -> device tensor of this processor's transform columns, in the reference's order"""
        at = {n: j for j, n in enumerate(names)}
        out: Dict[str, object] = {}
        for pre, own, ids, count, dates, n in (("u", self._unames, user, self._ucount, self._udates, self._n_users),
                                               ("i", self._inames, item, self._icount, self._idates, self._n_items)):
            for name in own:
                col = block[:, at[name]]
                out[name] = col.to(torch.int64) if name[2:] in _INT_COLS else col
                if name == f"{pre}_log_interact_days_count":
                    inside = (ids >= 0) & (ids < n)
                    safe = torch.where(inside, ids, torch.zeros_like(ids))
                    cold = ~inside | (count[safe] == 0)
                    for which, keys in zip(("min", "max"), dates):
                        out[f"{pre}_{which}_interact_date"] = torch.where(cold, torch.full_like(safe, _NAT), keys[safe])
        for name in ("na_u_log_features", "na_i_log_features", "u_i_log_num_interact_diff", "i_u_log_num_interact_diff"):
            out[name] = block[:, at[name]]
        return out

    def transform(self, log):
        if not self._fit_done:
            raise AttributeError("Call fit before running transform")
        return _transform(log, self, [], "LogStatFeaturesProcessor.transform")

    def transform_block(self, user_idx, item_idx, dtype=torch.float32):
        if not self._fit_done:
            raise AttributeError("Call fit before running transform")
        return _block(self, [], user_idx, item_idx, dtype)


class _PopFrames(dict):
    """conditional_pop_dict: the fitted device tables, turned into pandas frames when they are asked for"""

    def __init__(self, tables, entity_name):
        super().__init__(tables)
        self._entity = entity_name

    def __getitem__(self, col):
        import pandas as pd
        t = super().__getitem__(col)
        keys, n_cat = t["keys"].cpu().numpy(), t["n_cat"]
        code = keys % (n_cat + 1)
        cats = np.empty(len(code), dtype=object)
        cats[:] = [None if c == n_cat else t["uniques"][c] for c in code]
        return pd.DataFrame({self._entity: keys // (n_cat + 1), col: cats,
                             f"{self._entity[0]}_pop_by_{col}": t["pop"].cpu().numpy()})

    def table(self, col):
        return super().__getitem__(col)

    def values(self):
        return [self[k] for k in self]

    def items(self):
        return [(k, self[k]) for k in self]


def _features_frame(features):
    """`features` as a pandas frame on the host"""
    import pandas as pd
    if isinstance(features, pd.DataFrame):
        return features
    if isinstance(features, dict):
        return pd.DataFrame({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in features.items()})
    if hasattr(features, "to_pandas"):
        return features.to_pandas()
    import pyarrow as pa
    return pa.Table.from_batches(list(features)).to_pandas()


def _codes(values, uniques, n_cat: int) -> np.ndarray:
    """int32 code of every value: its index in `uniques`, n_cat for a null / NaN, -1 for a value fit did not see"""
    import pandas as pd
    values = pd.Series(values)
    code = pd.Index(uniques).get_indexer(values) if n_cat else np.full(len(values), -1)
    return np.where(values.isna().to_numpy(), n_cat, code).astype(np.int32)


class ConditionalPopularityProcessor(EmptyFeatureProcessor):
    """Popularity of an entity conditioned on a categorical feature of the other one (see the module docstring)."""

    conditional_pop_dict: Optional[Dict] = None
    entity_name: str

    def __init__(self, cat_features_list: List):
        self.cat_features_list = cat_features_list

    def fit(self, log, features) -> None:
        import pandas as pd
        feats = _features_frame(features)
        columns = list(feats.columns)
        if len(set(self.cat_features_list).intersection(columns)) != len(self.cat_features_list):
            raise ValueError(f"Columns {set(self.cat_features_list).difference(columns)} "
                             f"defined in `cat_features_list` are absent in features. "
                             f"features columns are: {columns}.")
        join_col, self.entity_name = (("item_idx", "user_idx") if "item_idx" in columns else ("user_idx", "item_idx"))
        src = L.normalise(log)
        for name in ("user_idx", "item_idx"):
            _id_column(src, name)
        fid = feats[join_col].to_numpy()
        if fid.dtype.kind not in "iu" or (len(fid) and (fid.min() < 0 or fid.max() >= (1 << 31) - 1)):
            raise ValueError(f"features column {join_col} must hold non-negative dense indices below 2^31 - 1")
        lg = L.open_log(src, "ConditionalPopularityProcessor.fit")
        feat = P.Feat(lg.device) if lg.n else None
        if lg.n:
            (entity, n_entity), (other, n_other) = L.dense_ids(lg, [self.entity_name, join_col])
            count = feat.count(entity, n_entity)
        else:
            n_entity = n_other = 0
        n_code = max(n_other, int(fid.max()) + 1 if len(fid) else 0)
        tables = {}
        for col in self.cat_features_list:
            codes, uniques = pd.factorize(feats[col])
            n_cat = len(uniques)
            per_id = np.full(n_code, n_cat, dtype=np.int32)
            per_id[fid] = np.where(codes < 0, n_cat, codes)
            code = torch.as_tensor(per_id).to(lg.device)
            if lg.n:
                keys, pop, off = feat.pair_counts(entity, other, code, count, n_entity, n_cat)
            else:
                keys = off = torch.zeros(0, dtype=torch.int64, device=lg.device)
                pop = torch.zeros(0, dtype=torch.float64, device=lg.device)
            tables[col] = {"code": code, "keys": keys, "pop": pop, "entity_off": off, "n_entity": n_entity, "n_cat": n_cat,
                           "uniques": list(uniques), "entity_is_item": self.entity_name == "item_idx"}
        self.conditional_pop_dict = _PopFrames(tables, self.entity_name)

    def _pops(self, lg=None):
        """([table dicts for the block kernel], the names of their columns)"""
        pops, names = [], []
        for col in self.conditional_pop_dict:
            t = dict(self.conditional_pop_dict.table(col))
            if lg is not None and col in lg.names:               # the frame's own category column wins
                if lg.kind == "device":
                    vals = lg.src[col].cpu().numpy() if torch.is_tensor(lg.src[col]) else lg.src[col]
                else:
                    vals = lg.src[col] if lg.kind == "pandas" else lg.table.column(col).to_pandas()
                t["pair_code"] = torch.as_tensor(_codes(vals, t["uniques"], t["n_cat"])).to(lg.device)
            pops.append(t)
            e = self.entity_name[0]
            names += [f"{e}_pop_by_{col}", f"na_{e}_pop_by_{col}"]
        return pops, names

    def transform(self, log):
        if self.conditional_pop_dict is None:
            raise AttributeError("Call fit before running transform")
        return _transform(log, None, [self], "ConditionalPopularityProcessor.transform")

    def transform_block(self, user_idx, item_idx, dtype=torch.float32):
        if self.conditional_pop_dict is None:
            raise AttributeError("Call fit before running transform")
        return _block(None, [self], user_idx, item_idx, dtype)


def _plan(log_proc, pop_procs, lg=None):
    """(colmap, names, popularity tables) of one block: the documented column order"""
    from . import _native as N
    colmap, names, pops = [], [], []
    if log_proc is not None:
        colmap, names = log_proc._block_parts()
        colmap, names = list(colmap), list(names)
    for proc in pop_procs:
        tabs, nms = proc._pops(lg)
        for t in tabs:
            colmap += [(N.FEATURES_COL_POP, len(pops), 0), (N.FEATURES_COL_POP_NA, len(pops), 0)]
            pops.append(t)
        names += nms
    return colmap, names, pops


def _launch(log_proc, pop_procs, user, item, dtype, lg=None):
    colmap, names, pops = _plan(log_proc, pop_procs, lg)
    if not colmap:
        return torch.empty((user.numel(), 0), dtype=dtype, device=user.device), names
    feat = P.Feat(user.device)
    if log_proc is not None and log_proc._n_users and log_proc._n_items:
        tabs = (log_proc._utab, log_proc._ucount, log_proc._itab, log_proc._icount)
    elif log_proc is not None:                        # fitted on an empty log: every id is cold
        tabs = (log_proc._utab, None, log_proc._itab, None)
    else:
        tabs = (None, None, None, None)
    return feat.block(user, item, tabs[0], tabs[1], tabs[2], tabs[3], colmap, pops, dtype), names


def _block(log_proc, pop_procs, user_idx, item_idx, dtype):
    from ._native import CqlrecError
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"a feature block is float32 or float64, not {dtype}")
    if not torch.cuda.is_available():
        raise CqlrecError("transform_block needs a GPU: it has no CPU path")
    if not (torch.is_tensor(user_idx) and torch.is_tensor(item_idx)) or user_idx.device.type != "cuda" or \
            item_idx.device != user_idx.device:
        raise CqlrecError("transform_block needs user_idx / item_idx as tensors on one GPU: it has no CPU path")
    if user_idx.dtype.is_floating_point or item_idx.dtype.is_floating_point or user_idx.shape != item_idx.shape or \
            user_idx.dim() != 1:
        raise ValueError("user_idx / item_idx must be integer vectors of one length")
    if user_idx.numel() >= L.MAX_ROWS:
        raise ValueError(f"a frame of {user_idx.numel()} pairs is beyond transform_block's 2^31 - 1")
    return _launch(log_proc, pop_procs, user_idx.to(torch.int64).contiguous(), item_idx.to(torch.int64).contiguous(), dtype)


def _transform(frame, log_proc, pop_procs, what: str):
    src = L.normalise(frame)
    for name in ("user_idx", "item_idx"):
        _id_column(src, name)
    lg = L.open_log(src, what)
    user, item = _pair_ids(lg)
    block, names = _launch(log_proc, pop_procs, user, item, torch.float64, lg)
    cols: Dict[str, object] = {}
    if log_proc is not None:
        cols.update(log_proc._frame_columns(block, names, user, item))
    for j, name in enumerate(names):
        if "_pop_by_" in name:
            cols[name] = block[:, j] != 0 if name.startswith("na_") else block[:, j]
    return _append(lg, cols, log_proc is not None and log_proc._ts_kind == "datetime")


# pylint: disable=too-many-instance-attributes, too-many-arguments
class HistoryBasedFeaturesProcessor:
    """LogStatFeaturesProcessor and ConditionalPopularityProcessor as a pipeline (see the module docstring)."""

    def __init__(self, use_log_features: bool = True, use_conditional_popularity: bool = True,
                 user_cat_features_list: Optional[List] = None, item_cat_features_list: Optional[List] = None):
        self.log_processor = EmptyFeatureProcessor()
        self.user_cond_pop_proc = EmptyFeatureProcessor()
        self.item_cond_pop_proc = EmptyFeatureProcessor()
        if use_log_features:
            self.log_processor = LogStatFeaturesProcessor()
        if use_conditional_popularity and user_cat_features_list:
            self.user_cond_pop_proc = ConditionalPopularityProcessor(cat_features_list=user_cat_features_list)
        if use_conditional_popularity and item_cat_features_list:
            self.item_cond_pop_proc = ConditionalPopularityProcessor(cat_features_list=item_cat_features_list)
        self.fitted: bool = False

    def fit(self, log, user_features=None, item_features=None) -> None:
        log = L.normalise(log)
        self.log_processor.fit(log=log, features=user_features)
        self.user_cond_pop_proc.fit(log=log, features=user_features)
        self.item_cond_pop_proc.fit(log=log, features=item_features)
        self.fitted = True

    def _parts(self):
        log_proc = self.log_processor if isinstance(self.log_processor, LogStatFeaturesProcessor) else None
        pops = [p for p in (self.user_cond_pop_proc, self.item_cond_pop_proc)
                if isinstance(p, ConditionalPopularityProcessor)]
        return log_proc, pops

    def transform(self, log):
        if not self.fitted:
            raise AttributeError("Call fit before running transform")
        log_proc, pops = self._parts()
        if log_proc is None and not pops:
            return log
        return _transform(log, log_proc, pops, "HistoryBasedFeaturesProcessor.transform")

    def transform_block(self, user_idx, item_idx, dtype=torch.float32):
        """(block [n_pairs, F] of `dtype` on the device, the names of its F columns): one launch, no host sync"""
        if not self.fitted:
            raise AttributeError("Call fit before running transform")
        log_proc, pops = self._parts()
        return _block(log_proc, pops, user_idx, item_idx, dtype)
