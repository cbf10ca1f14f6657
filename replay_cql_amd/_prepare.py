"""What filters.py and indexer.py share: a look at a log's columns that needs no GPU, and the calls into
csrc/prepare.hip (section f6 of include/cqlrec.h).  The log itself is splitters._Log, unchanged."""
from __future__ import annotations

import numpy as np
import torch

from . import data as D
from .splitters import _Log

MAX_ROWS = 1 << 31
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def clip64(x: int) -> int:
    return max(I64_MIN, min(I64_MAX, int(x)))


def normalise(log):
    """A one-shot iterable of record batches is read once, into a list that can be looked at twice."""
    if isinstance(log, dict) or hasattr(log, "columns") or hasattr(log, "schema"):
        return log
    try:
        return list(log)
    except TypeError:
        return log                                    # _Log names the kinds it takes


def has_column(log, name: str) -> bool:
    if isinstance(log, dict):
        return name in log
    if hasattr(log, "iloc"):
        return name in log.columns
    schema = getattr(log, "schema", None) or (log[0].schema if isinstance(log, list) and log and
                                              hasattr(log[0], "schema") else None)
    return schema is not None and name in schema.names


def column_kind(log, name: str):
    """(numpy dtype kind of column `name`, its dtype: torch's for a dict of tensors, numpy's or None otherwise) of a
    normalised log, read on the host from the frame's own schema; ValueError if the column is missing."""
    if isinstance(log, dict):
        if name not in log:
            raise ValueError(f"log has no column {name}")
        t = log[name]
        if not torch.is_tensor(t):
            raise ValueError(f"column {name} is no tensor")
        kind = "f" if t.dtype.is_floating_point else "b" if t.dtype == torch.bool else "i"
        return kind, t.dtype
    if hasattr(log, "columns") and hasattr(log, "iloc"):                   # pandas
        if name not in log.columns:
            raise ValueError(f"log has no column {name}")
        dt = log[name].dtype
        return (dt.kind, dt) if isinstance(dt, np.dtype) else ("O", None)
    schema = log.schema if hasattr(log, "schema") else (log[0].schema if isinstance(log, list) and log and
                                                        hasattr(log[0], "schema") else None)
    if schema is None:
        raise ValueError(f"cannot read a log of type {type(log)}: pandas, pyarrow or a dict of tensors")
    if name not in schema.names:
        raise ValueError(f"log has no column {name}")
    import pyarrow as pa
    ty = schema.field(name).type
    if pa.types.is_integer(ty):
        dt = np.dtype(ty.to_pandas_dtype())
        return dt.kind, dt
    if pa.types.is_floating(ty):
        return "f", np.dtype(ty.to_pandas_dtype())
    if pa.types.is_timestamp(ty) or pa.types.is_date(ty):
        return "M", None
    if pa.types.is_boolean(ty):
        return "b", np.dtype(bool)
    return "O", None


def open_log(log, what: str) -> _Log:
    """splitters._Log of a normalised log, on a GPU: CqlrecError without one, ValueError beyond 2^31 - 1 rows."""
    from ._native import CqlrecError
    if not torch.cuda.is_available():
        raise CqlrecError(f"{what} needs a GPU: it has no CPU path")
    lg = _Log(log)
    if lg.device.type != "cuda":
        raise CqlrecError(f"{what} needs the columns on a GPU: it has no CPU path")
    if lg.n >= MAX_ROWS:
        raise ValueError(f"a log of {lg.n} rows is beyond {what}'s 2^31 - 1")
    return lg


def float_column(lg: _Log, name: str):
    if lg.kind == "device":
        return lg.src[name].to(torch.float64).contiguous()
    return D._dev_col(lg._host(name).astype(np.float64, copy=False), torch.float64, lg.device)


def dense_ids(lg: _Log, names):
    """[(int32 device ids, largest id + 1)] of the integer columns `names`, range-checked in one small sync."""
    cols = [lg.ids(nm) for nm in names]
    lim = torch.stack([f(c) for c in cols for f in (torch.min, torch.max)]).cpu().tolist()
    if min(lim[0::2]) < 0:
        raise ValueError(f"{' / '.join(names)} must be non-negative dense indices")
    if max(lim[1::2]) >= (1 << 31) - 1:
        raise ValueError(f"{' / '.join(names)} must be below 2^31 - 1")
    return [(c.to(torch.int32), int(hi) + 1) for c, hi in zip(cols, lim[1::2])]


class Prep:
    """The calls into csrc/prepare.hip on one device."""

    def __init__(self, device):
        from . import _native as N
        self.N, self.lib, self.dev = N, N.load(), device
        self.stream = torch.cuda.current_stream(device).cuda_stream

    def _empty(self, n, dt):
        return torch.empty(int(n), dtype=dt, device=self.dev)

    def _ws(self, nbytes: int):
        return self._empty(nbytes, torch.uint8)

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    def rank(self, user, n_users: int, key, key2=None, n_key2: int = 0):
        """(rank int32[n], count int32[n_users]) under (key desc, key2 desc, row desc) -- cqlrec_prepare_rank"""
        n = user.numel()
        rank, count = self._empty(n, torch.int32), self._empty(n_users, torch.int32)
        nb = int(self.lib.cqlrec_prepare_rank_ws_bytes(n, n_users))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_prepare_rank(user.data_ptr(), key.data_ptr(), self._p(key2), n, n_users, int(n_key2),
                                                  ws.data_ptr(), nb, rank.data_ptr(), count.data_ptr(), self.stream),
                     "prepare_rank")
        return rank, count

    def count(self, ids, n_groups: int):
        out = self._empty(n_groups, torch.int32)
        self.N.check(self.lib.cqlrec_prepare_count(ids.data_ptr(), ids.numel(), n_groups, out.data_ptr(), self.stream),
                     "prepare_count")
        return out

    def minmax(self, group, n_groups: int, key):
        lo, hi = self._empty(n_groups, torch.int64), self._empty(n_groups, torch.int64)
        self.N.check(self.lib.cqlrec_prepare_minmax(self._p(group), key.data_ptr(), key.numel(), n_groups, lo.data_ptr(),
                                                    hi.data_ptr(), self.stream), "prepare_minmax")
        return lo, hi

    def keep(self, rule: int, n_rows: int, group=None, key=None, value=None, rank=None, count=None, extreme=None, n: int = 0,
             first: bool = True, float_key: bool = False, lo: int = 0, hi: int = 0, open_end: bool = False, x: float = 0.0):
        out = self._empty(n_rows, torch.uint8)
        self.N.check(self.lib.cqlrec_prepare_keep(rule, self._p(group), self._p(key), self._p(value), self._p(rank),
                                                  self._p(count), self._p(extreme), n_rows, int(n), int(first),
                                                  int(float_key), int(lo), int(hi), int(open_end), float(x), out.data_ptr(),
                                                  self.stream), "prepare_keep")
        return out

    def compact(self, keep):
        n = keep.numel()
        rows, kept = self._empty(n, torch.int64), self._empty(1, torch.int64)
        nb = int(self.lib.cqlrec_prepare_compact_ws_bytes(n))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_prepare_compact(keep.data_ptr(), n, ws.data_ptr(), nb, rows.data_ptr(), kept.data_ptr(),
                                                     self.stream), "prepare_compact")
        return rows[:int(kept.item())]                       # the one device-to-host sync of a filter proper

    def distinct(self, ids):
        n = ids.numel()
        out, m = self._empty(n, torch.int64), self._empty(1, torch.int64)
        nb = int(self.lib.cqlrec_prepare_distinct_ws_bytes(n))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_prepare_distinct(ids.data_ptr(), n, ws.data_ptr(), nb, out.data_ptr(), m.data_ptr(),
                                                      self.stream), "prepare_distinct")
        return out[:int(m.item())].clone()

    def sort_labels(self, labels):
        m = labels.numel()
        srt, idx = self._empty(m, torch.int64), self._empty(m, torch.int32)
        nb = int(self.lib.cqlrec_prepare_sort_labels_ws_bytes(m))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_prepare_sort_labels(labels.data_ptr(), m, ws.data_ptr(), nb, srt.data_ptr(),
                                                         idx.data_ptr(), self.stream), "prepare_sort_labels")
        return srt, idx

    def lookup(self, ids, srt, idx):
        """(int32 label index per row, -1 where the id is unknown; whether any was)"""
        out, miss = self._empty(ids.numel(), torch.int32), self._empty(1, torch.int32)
        self.N.check(self.lib.cqlrec_prepare_lookup(ids.data_ptr(), ids.numel(), srt.data_ptr(), idx.data_ptr(), srt.numel(),
                                                    out.data_ptr(), miss.data_ptr(), self.stream), "prepare_lookup")
        return out, bool(miss.item())

    def gather(self, idx, labels):
        out, bad = self._empty(idx.numel(), torch.int64), self._empty(1, torch.int32)
        self.N.check(self.lib.cqlrec_prepare_gather(idx.data_ptr(), idx.numel(), labels.data_ptr(), labels.numel(),
                                                    out.data_ptr(), bad.data_ptr(), self.stream), "prepare_gather")
        return out, bool(bad.item())


class Feat(Prep):
    """The calls into csrc/features.hip (section f7 of include/cqlrec.h) on one device."""

    def day(self, key, unit: int):
        out = self._empty(key.numel(), torch.int64)
        self.N.check(self.lib.cqlrec_features_day(key.data_ptr(), key.numel(), int(unit), out.data_ptr(), self.stream),
                     "features_day")
        return out

    def segments(self, group, n_groups: int, key=None):
        """(perm int32[n], offsets int64[n_groups + 1]) of the rows ordered by (group, key, row) ascending"""
        n = group.numel()
        perm, offsets = self._empty(n, torch.int32), self._empty(n_groups + 1, torch.int64)
        nb = int(self.lib.cqlrec_features_segments_ws_bytes(n, n_groups))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_features_segments(group.data_ptr(), self._p(key), n, n_groups, ws.data_ptr(), nb,
                                                       perm.data_ptr(), offsets.data_ptr(), self.stream),
                     "features_segments")
        return perm, offsets

    def segment_stats(self, perm, offsets, value, n_groups: int):
        """float64 [n_groups, 6]: count, mean, std, quantile_05, quantile_5, quantile_95"""
        n = perm.numel()
        out = torch.empty((n_groups, self.N.FEATURES_STATS), dtype=torch.float64, device=self.dev)
        nb = int(self.lib.cqlrec_features_segment_stats_ws_bytes(n, n_groups))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_features_segment_stats(perm.data_ptr(), offsets.data_ptr(), value.data_ptr(), n,
                                                            n_groups, ws.data_ptr(), nb, out.data_ptr(), self.stream),
                     "features_segment_stats")
        return out

    def segment_mean(self, rule: int, perm, offsets, n_groups: int, other, tab_a, tab_b=None, value=None,
                     min_std: float = 0.0, max_std: float = 0.0):
        """float64 [n_groups]: the mean over the group's rows; tab_a / tab_b are columns of ONE row-major table"""
        n = perm.numel()
        out = self._empty(n_groups, torch.float64)
        stride = int(tab_a.stride(0)) if tab_a.numel() else 1
        if tab_b is not None and tab_b.numel() and int(tab_b.stride(0)) != stride:
            raise ValueError("tab_a and tab_b differ in stride")
        nb = int(self.lib.cqlrec_features_segment_mean_ws_bytes(n, n_groups))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_features_segment_mean(rule, perm.data_ptr(), offsets.data_ptr(), self._p(value),
                                                           other.data_ptr(), tab_a.data_ptr(), self._p(tab_b), stride,
                                                           float(min_std), float(max_std), n, n_groups, ws.data_ptr(), nb,
                                                           out.data_ptr(), self.stream), "features_segment_mean")
        return out

    def segment_distinct(self, group, perm, offsets, key, n_groups: int):
        out = self._empty(n_groups, torch.int32)
        self.N.check(self.lib.cqlrec_features_segment_distinct(group.data_ptr(), perm.data_ptr(), offsets.data_ptr(),
                                                               key.data_ptr(), perm.numel(), n_groups, out.data_ptr(),
                                                               self.stream), "features_segment_distinct")
        return out

    def pair_counts(self, entity, other, code, entity_count, n_entity: int, n_cat: int):
        """(sorted distinct keys int64[m], popularity float64[m], first key of every entity int64[n_entity + 1])"""
        n = entity.numel()
        keys, pop, m = self._empty(n, torch.int64), self._empty(n, torch.float64), self._empty(1, torch.int64)
        off = self._empty(n_entity + 1, torch.int64)
        nb = int(self.lib.cqlrec_features_pair_counts_ws_bytes(n))
        ws = self._ws(nb)
        self.N.check(self.lib.cqlrec_features_pair_counts(entity.data_ptr(), other.data_ptr(), code.data_ptr(),
                                                          entity_count.data_ptr(), n, n_entity, n_cat, ws.data_ptr(), nb,
                                                          keys.data_ptr(), pop.data_ptr(), off.data_ptr(), m.data_ptr(),
                                                          self.stream), "features_pair_counts")
        m = int(m.item())
        return keys[:m].clone(), pop[:m].clone(), off

    def block(self, user, item, utab, ucount, itab, icount, colmap, pops, dtype):
        """[n_pairs, len(colmap)] of `dtype` in one launch.  utab / itab: float64 [n, f] or None; colmap: (kind, a, b)
        triples; pops: dicts with code, pair_code, keys, pop, entity_off, n_entity, n_cat, entity_is_item."""
        import ctypes as C
        N = self.N
        n, f = user.numel(), len(colmap)
        if not 0 < f <= N.FEATURES_MAX_COLS or len(pops) > N.FEATURES_MAX_POP:
            raise ValueError(f"a feature block takes 1..{N.FEATURES_MAX_COLS} columns and at most {N.FEATURES_MAX_POP} "
                             f"conditional-popularity tables, not {f} and {len(pops)}")
        out = torch.empty((n, f), dtype=dtype, device=self.dev)
        cm = (C.c_int32 * (3 * f))(*[int(x) for t in colmap for x in t])
        ps = (N.FeaturesPop * max(1, len(pops)))()
        for q, d in enumerate(pops):
            ps[q] = N.FeaturesPop(self._p(d["code"]), self._p(d.get("pair_code")), self._p(d["keys"]), self._p(d["pop"]),
                                  self._p(d["entity_off"]), d["code"].numel(), int(d["n_entity"]), int(d["n_cat"]), d["keys"].numel(),
                                  int(d["entity_is_item"]), 0)
        nu, fu = (0, 0) if utab is None else utab.shape
        ni, fi = (0, 0) if itab is None else itab.shape
        N.check(self.lib.cqlrec_features_block(user.data_ptr(), item.data_ptr(), n, self._p(utab), self._p(ucount), int(nu),
                                               int(fu), self._p(itab), self._p(icount), int(ni), int(fi), cm, f, ps,
                                               len(pops), 0 if dtype == torch.float32 else 1, out.data_ptr(), self.stream),
                "features_block")
        return out
