"""The calls into csrc/prepare.hip and csrc/features.hip (sections f6 and f7 of include/cqlrec.h) that filters.py,
indexer.py, history_based_fp.py and the device-fitted models share; `Feat.view` is the one builder of a CSR view of the
log."""
from __future__ import annotations

from typing import Optional

import torch

from ._device import Engine, Ws, _ptr


def count_pieces(offsets: torch.Tensor, rows: Optional[torch.Tensor] = None, piece: int = 1024) -> int:
    """the `n_pieces` argument of the row entry points of csrc/als.hip and csrc/dense.hip (CQLREC_ALS_PIECE and
    CQLREC_DENSE_GRAM_PIECE are both 1024): the pieces of the (listed) rows longer than one piece"""
    lens = offsets[1:] - offsets[:-1]
    if rows is not None:
        lens = lens[rows.long()]
    long = lens[lens > piece]
    return int(((long + piece - 1) // piece).sum().item()) if long.numel() else 0


class Prep(Engine):
    """The calls into csrc/prepare.hip on one device."""

    def rank(self, user, n_users: int, key, key2=None, n_key2: int = 0):
        """(rank int32[n], count int32[n_users]) under (key desc, key2 desc, row desc) -- cqlrec_prepare_rank"""
        n = user.numel()
        rank, count = self._empty(n, torch.int32), self._empty(n_users, torch.int32)
        self.call("prepare_rank", user, key, key2, n, n_users, int(n_key2), Ws(n, n_users), rank, count)
        return rank, count

    def count(self, ids, n_groups: int):
        out = self._empty(n_groups, torch.int32)
        self.call("prepare_count", ids, ids.numel(), n_groups, out)
        return out

    def minmax(self, group, n_groups: int, key):
        lo, hi = self._empty(n_groups, torch.int64), self._empty(n_groups, torch.int64)
        self.call("prepare_minmax", group, key, key.numel(), n_groups, lo, hi)
        return lo, hi

    def keep(self, rule: int, n_rows: int, group=None, key=None, value=None, rank=None, count=None, extreme=None, n: int = 0,
             first: bool = True, float_key: bool = False, lo: int = 0, hi: int = 0, open_end: bool = False, x: float = 0.0):
        out = self._empty(n_rows, torch.uint8)
        self.call("prepare_keep", rule, group, key, value, rank, count, extreme, n_rows, int(n), int(first), int(float_key),
                  int(lo), int(hi), int(open_end), float(x), out)
        return out

    def compact(self, keep):
        n = keep.numel()
        rows, kept = self._empty(n, torch.int64), self._empty(1, torch.int64)
        self.call("prepare_compact", keep, n, Ws(n), rows, kept)
        return rows[:int(kept.item())]                       # the one device-to-host sync of a filter proper

    def distinct(self, ids):
        n = ids.numel()
        out, m = self._empty(n, torch.int64), self._empty(1, torch.int64)
        self.call("prepare_distinct", ids, n, Ws(n), out, m)
        return out[:int(m.item())].clone()

    def sort_labels(self, labels):
        m = labels.numel()
        srt, idx = self._empty(m, torch.int64), self._empty(m, torch.int32)
        self.call("prepare_sort_labels", labels, m, Ws(m), srt, idx)
        return srt, idx

    def lookup(self, ids, srt, idx):
        """(int32 label index per row, -1 where the id is unknown; whether any was)"""
        out, miss = self._empty(ids.numel(), torch.int32), self._empty(1, torch.int32)
        self.call("prepare_lookup", ids, ids.numel(), srt, idx, srt.numel(), out, miss)
        return out, bool(miss.item())

    def gather(self, idx, labels):
        out, bad = self._empty(idx.numel(), torch.int64), self._empty(1, torch.int32)
        self.call("prepare_gather", idx, idx.numel(), labels, labels.numel(), out, bad)
        return out, bool(bad.item())


class Feat(Prep):
    """The calls into csrc/features.hip (section f7 of include/cqlrec.h) on one device."""

    def day(self, key, unit: int):
        out = self._empty(key.numel(), torch.int64)
        self.call("features_day", key, key.numel(), int(unit), out)
        return out

    def segments(self, group, n_groups: int, key=None):
        """(perm int32[n], offsets int64[n_groups + 1]) of the rows ordered by (group, key, row) ascending"""
        n = group.numel()
        perm, offsets = self._empty(n, torch.int32), self._empty(n_groups + 1, torch.int64)
        self.call("features_segments", group, key, n, n_groups, Ws(n, n_groups), perm, offsets)
        return perm, offsets

    def view(self, group, n_groups: int, other, weight=None):
        """A view of the log: its rows ordered by (group, other id, row) as the CSR triple (offsets int64 [n_groups + 1],
        other id [n], weight [n] or None), and the int32 permutation that orders them"""
        perm, offsets = self.segments(group, n_groups, other.to(torch.int64))
        rows = perm.long()
        return (offsets, other[rows].contiguous(), None if weight is None else weight[rows].contiguous()), perm

    def segment_stats(self, perm, offsets, value, n_groups: int):
        """float64 [n_groups, 6]: count, mean, std, quantile_05, quantile_5, quantile_95"""
        n = perm.numel()
        out = torch.empty((n_groups, self.N.FEATURES_STATS), dtype=torch.float64, device=self.dev)
        self.call("features_segment_stats", perm, offsets, value, n, n_groups, Ws(n, n_groups), out)
        return out

    def segment_mean(self, rule: int, perm, offsets, n_groups: int, other, tab_a, tab_b=None, value=None,
                     min_std: float = 0.0, max_std: float = 0.0):
        """float64 [n_groups]: the mean over the group's rows; tab_a / tab_b are columns of ONE row-major table"""
        n = perm.numel()
        out = self._empty(n_groups, torch.float64)
        stride = int(tab_a.stride(0)) if tab_a.numel() else 1
        if tab_b is not None and tab_b.numel() and int(tab_b.stride(0)) != stride:
            raise ValueError("tab_a and tab_b differ in stride")
        self.call("features_segment_mean", rule, perm, offsets, value, other, tab_a, tab_b, stride, float(min_std),
                  float(max_std), n, n_groups, Ws(n, n_groups), out)
        return out

    def segment_distinct(self, group, perm, offsets, key, n_groups: int):
        out = self._empty(n_groups, torch.int32)
        self.call("features_segment_distinct", group, perm, offsets, key, perm.numel(), n_groups, out)
        return out

    def pair_counts(self, entity, other, code, entity_count, n_entity: int, n_cat: int):
        """(sorted distinct keys int64[m], popularity float64[m], first key of every entity int64[n_entity + 1])"""
        n = entity.numel()
        keys, pop, m = self._empty(n, torch.int64), self._empty(n, torch.float64), self._empty(1, torch.int64)
        off = self._empty(n_entity + 1, torch.int64)
        self.call("features_pair_counts", entity, other, code, entity_count, n, n_entity, n_cat, Ws(n), keys, pop, off, m)
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
            ps[q] = N.FeaturesPop(_ptr(d["code"]), _ptr(d.get("pair_code")), _ptr(d["keys"]), _ptr(d["pop"]),
                                  _ptr(d["entity_off"]), d["code"].numel(), int(d["n_entity"]), int(d["n_cat"]), d["keys"].numel(),
                                  int(d["entity_is_item"]), 0)
        nu, fu = (0, 0) if utab is None else utab.shape
        ni, fi = (0, 0) if itab is None else itab.shape
        self.call("features_block", user, item, n, utab, ucount, int(nu), int(fu), itab, icount, int(ni), int(fi), cm, f, ps,
                  len(pops), 0 if dtype == torch.float32 else 1, out)
        return out
