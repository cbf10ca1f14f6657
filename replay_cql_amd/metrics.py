"""On-device evaluation.

`evaluate_topk`: NDCG / HitRate / Precision / Recall / MAP / MRR @ k of a top-k block with the reference's per-user
formulas (replay/metrics/*.py) and user set (replay/metrics/base_metric.py:102-140), so that optimize()-style loops
(replay/optuna_objective.py:80-111) keep the U x k result on the GPU.

The metric classes below evaluate any recommendation FRAME -- a baseline, a loaded parquet file, another model's output
-- with the call signatures of replay/metrics: the frame becomes a block on the device (csrc/metrics.hip: get_top_k_recs
+ sorter), the six metrics above come from `evaluate_topk`, RocAuc / Unexpectedness / Surprisal / NCISPrecision from
cqlrec_eval_extras, Coverage and item_distribution from the item-side kernels.  Frames are pandas, pyarrow (through
arrow_io.columns_to_device) or a dict of device tensors.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from statistics import NormalDist
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _native as N
from ._device import Engine, Ws

METRICS = ("NDCG", "HitRate", "Precision", "Recall", "MAP", "MRR")


def _eval_topk_sums(rec_idx: torch.Tensor, gt_offsets: torch.Tensor, gt_items: torch.Tensor, ks: List[int],
                    rec_rows: Optional[torch.Tensor], return_per_user: bool):
    """cqlrec_eval_topk: (sums float64 [6 x n_ks] on the host, per_user [n x 6 x n_ks] on the device or None)."""
    n, kmax = int(rec_idx.shape[0]), int(rec_idx.shape[1])
    dev = rec_idx.device
    rec_idx = rec_idx.to(torch.int32).contiguous()
    sums = torch.zeros(len(METRICS) * len(ks), dtype=torch.float64, device=dev)
    per_user = torch.empty((n, len(METRICS), len(ks)), dtype=torch.float64, device=dev) if return_per_user else None
    Engine(dev).call("eval_topk", rec_idx, n, kmax, rec_rows, gt_offsets, gt_items, (C.c_int32 * len(ks))(*ks), len(ks),
                     Ws(n, len(ks)), per_user, sums)
    return sums.cpu().numpy().reshape(len(METRICS), len(ks)), per_user


def evaluate_topk(rec_idx: torch.Tensor, gt_offsets: torch.Tensor, gt_items: torch.Tensor, ks: Iterable[int],
                  rec_rows: Optional[torch.Tensor] = None, n_gt_users: Optional[int] = None,
                  return_per_user: bool = False):
    """rec_idx int32 [n x kmax] (-1 padded, best first); ground-truth CSR with ascending unique items per row; row u of
    rec_idx is evaluated against CSR row rec_rows[u] (default u).  Returns {metric: {k: mean over n_gt_users}}."""
    ks = sorted(int(k) for k in ks)
    n = int(rec_idx.shape[0])
    sums, per_user = _eval_topk_sums(rec_idx, gt_offsets, gt_items, ks, rec_rows, return_per_user)
    denom = float(n if n_gt_users is None else n_gt_users)
    vals = sums / denom
    out: Dict[str, Dict[int, float]] = {m: {k: float(vals[mi, ki]) for ki, k in enumerate(ks)}
                                        for mi, m in enumerate(METRICS)}
    return (out, per_user) if return_per_user else out


# =====================================================================================================================
# device primitives (csrc/metrics.hip)
# =====================================================================================================================
EXTRAS = N.EVAL_EXTRAS
_ACTIVATIONS = {None: N.NCIS_NONE, "logit": N.NCIS_SIGMOID, "sigmoid": N.NCIS_SIGMOID, "softmax": N.NCIS_SOFTMAX}


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise N.CqlrecError("replay_cql_amd.metrics evaluates on the GPU: there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _ks_list(k) -> List[int]:
    ks = sorted({int(x) for x in ([k] if isinstance(k, (int, np.integer)) else k)})
    if not ks or ks[0] <= 0 or len(ks) > 8:
        raise ValueError(f"k: between one and eight positive cut-offs, got {k}")
    return ks


def frame_to_block(row: torch.Tensor, item: torch.Tensor, rel: torch.Tensor, n_users: int, kmax: int,
                   dedup: bool = True, payload: Optional[torch.Tensor] = None, want_val: bool = False,
                   want_pos: bool = False):
    """Frame columns on the device -> (rec_idx, rec_val, rec_pos, rec_w), each [n_users x kmax] or None
    (cqlrec_recs_frame_to_block).  `row` int32: the frame row's index into the evaluated users, anything outside
    0..n_users-1 for a user that is not evaluated."""
    dev = item.device
    n_rows = int(item.numel())
    if n_rows and bool(torch.isnan(rel).any()):
        raise ValueError("relevance contains NaN")
    if n_rows and int(item.min()) < 0:
        raise ValueError("item_idx must be non-negative")
    rec = torch.empty((n_users, kmax), dtype=torch.int32, device=dev)
    val = torch.empty((n_users, kmax), dtype=torch.float64, device=dev) if want_val else None
    pos = torch.empty((n_users, kmax), dtype=torch.int32, device=dev) if want_pos else None
    w = torch.empty((n_users, kmax), dtype=torch.float64, device=dev) if payload is not None else None
    Engine(dev).call("recs_frame_to_block", row, item, rel, payload, n_rows, n_users, kmax, int(bool(dedup)),
                     Ws(n_rows, n_users), rec, val, pos, w)
    return rec, val, pos, w


def evaluate_extras(rec_idx: torch.Tensor, ks: Sequence[int], gt_offsets: Optional[torch.Tensor] = None,
                    gt_items: Optional[torch.Tensor] = None, rec_rows: Optional[torch.Tensor] = None,
                    base_idx: Optional[torch.Tensor] = None, item_w: Optional[torch.Tensor] = None,
                    rec_w: Optional[torch.Tensor] = None):
    """(sums float64 [4 x n_ks] on the host, per_user float64 [n x 4 x n_ks] on the device) in the order of EXTRAS
    (cqlrec_eval_extras); a metric whose input is absent comes out 0."""
    ks = [int(k) for k in ks]
    n, kmax = int(rec_idx.shape[0]), int(rec_idx.shape[1])
    dev = rec_idx.device
    sums = torch.zeros(len(EXTRAS) * len(ks), dtype=torch.float64, device=dev)
    per_user = torch.empty((n, len(EXTRAS), len(ks)), dtype=torch.float64, device=dev)
    Engine(dev).call("eval_extras", rec_idx, n, kmax, rec_rows, gt_offsets, gt_items, base_idx,
                     0 if base_idx is None else int(base_idx.shape[1]), item_w, 0 if item_w is None else int(item_w.numel()),
                     rec_w, (C.c_int32 * len(ks))(*ks), len(ks), Ws(n, len(ks)), per_user, sums)
    return sums.cpu().numpy().reshape(len(EXTRAS), len(ks)), per_user


def item_user_counts(item: torch.Tensor, user: torch.Tensor, n_items: int):
    """(distinct users per item int32 [n_items], distinct users of the log) -- cqlrec_eval_item_user_counts."""
    dev = item.device
    n_rows = int(item.numel())
    cnt = torch.zeros(n_items, dtype=torch.int32, device=dev)
    if n_rows == 0:
        return cnt, 0
    nu = torch.zeros(1, dtype=torch.int64, device=dev)
    Engine(dev).call("eval_item_user_counts", item, user, n_rows, n_items, Ws(n_rows), cnt, nu)
    return cnt, int(nu.item())


def surprisal_weights(item: torch.Tensor, user: torch.Tensor) -> torch.Tensor:
    """Per-item self-information of a log, normalised (replay/metrics/surprisal.py:57-63): float64 [max item + 1]."""
    if int(item.numel()) == 0:
        raise ValueError("Surprisal needs a log with at least two users")
    n_items = int(item.max()) + 1
    cnt, n_users = item_user_counts(item, user, n_items)
    if n_users < 2:
        raise ValueError("Surprisal needs a log with at least two users: log2(1) = 0 leaves the weights undefined")
    w = torch.empty(n_items, dtype=torch.float64, device=item.device)
    Engine(item.device).call("eval_surprisal_weights", cnt, n_items, n_users, w)
    return w


def coverage_counts(rec_idx: torch.Tensor, rec_pos: torch.Tensor, ks: Sequence[int]) -> List[int]:
    """For each k: how many items have a best position <= k (cqlrec_eval_coverage)."""
    ks = [int(k) for k in ks]
    n, kmax = int(rec_idx.shape[0]), int(rec_idx.shape[1])
    n_items = int(rec_idx.max()) + 1 if n else 0
    if n_items <= 0:
        return [0] * len(ks)
    dev = rec_idx.device
    best = torch.empty(n_items, dtype=torch.int32, device=dev)
    counts = torch.zeros(len(ks), dtype=torch.int64, device=dev)
    Engine(dev).call("eval_coverage", rec_idx, rec_pos, n, kmax, n_items, (C.c_int32 * len(ks))(*ks), len(ks), best, counts)
    return [int(c) for c in counts.cpu().tolist()]


# =====================================================================================================================
# frames
# =====================================================================================================================
def _column(x, dev, dtype) -> torch.Tensor:
    if torch.is_tensor(x):
        return x.to(device=dev, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x))).to(device=dev, dtype=dtype).contiguous()


def _columns(frame, dev, need_rel: bool = False, need_user: bool = True) -> Dict[str, Optional[torch.Tensor]]:
    """{user_idx int32, item_idx int32, relevance float64 | None} on the device, from pandas / pyarrow / dict."""
    import pyarrow as pa
    if isinstance(frame, (pa.Table, pa.RecordBatch)):
        from . import arrow_io as A
        if frame.num_rows == 0:
            cols = {c: None for c in frame.schema.names}
        else:
            names = [c for c in ("user_idx", "item_idx", "relevance") if c in frame.schema.names]
            cols = dict(A.columns_to_device(frame.select(names), dev, names))
    elif isinstance(frame, dict):
        cols = dict(frame)
    else:                                               # pandas
        cols = {c: frame[c].to_numpy() for c in ("user_idx", "item_idx", "relevance") if c in frame.columns}
    out: Dict[str, Optional[torch.Tensor]] = {}
    for name, dt in (("user_idx", torch.int32), ("item_idx", torch.int32), ("relevance", torch.float64)):
        v = cols.get(name)
        out[name] = None if v is None else _column(v, dev, dt)
    n = 0 if out["item_idx"] is None else int(out["item_idx"].numel())
    if out["item_idx"] is None:
        out["item_idx"] = torch.zeros(0, dtype=torch.int32, device=dev)
    if out["user_idx"] is None:
        if need_user and n:
            raise ValueError("frame has no column user_idx")
        out["user_idx"] = None if n else torch.zeros(0, dtype=torch.int32, device=dev)
    if out["relevance"] is None:
        if need_rel and n:
            raise ValueError("frame has no column relevance")
        out["relevance"] = torch.zeros(n, dtype=torch.float64, device=dev) if need_rel else None
    return out


def _users(x, dev) -> torch.Tensor:
    """ground_truth_users: a frame with user_idx, or ids -> ascending unique int64 on the device."""
    import pandas as pd
    import pyarrow as pa
    from . import arrow_io as A
    if isinstance(x, pd.DataFrame):
        x = x["user_idx"].to_numpy()
    elif isinstance(x, dict):
        x = x["user_idx"]
    elif isinstance(x, (pa.Table, pa.RecordBatch)) and x.num_rows == 0:
        x = np.zeros(0, np.int64)
    return A.ids_to_device(x, "user_idx", dev)


def _rows_of(users: torch.Tensor, user_col: torch.Tensor) -> torch.Tensor:
    """index of each frame row's user in the ascending `users`, -1 where it is not one of them (int32)."""
    if users.numel() == 0 or user_col.numel() == 0:
        return torch.full((int(user_col.numel()),), -1, dtype=torch.int32, device=user_col.device)
    u = user_col.to(torch.int64)
    r = torch.searchsorted(users, u).clamp_(max=int(users.numel()) - 1)
    return torch.where(users[r] == u, r, torch.full_like(r, -1)).to(torch.int32)


def _gt_csr(gt: Dict[str, torch.Tensor], users: torch.Tensor):
    """ground truth -> CSR over `users` (collect_set: items ascending, unique); one padding item keeps the array
    non-empty."""
    dev = users.device
    n = int(users.numel())
    rows = _rows_of(users, gt["user_idx"]).to(torch.int64)
    keep = rows >= 0
    key = torch.unique((rows[keep] << 32) | gt["item_idx"][keep].to(torch.int64))
    r = key >> 32
    off = torch.searchsorted(r, torch.arange(n + 1, device=dev, dtype=torch.int64)).to(torch.int64).contiguous()
    items = torch.cat([(key & 0xFFFFFFFF).to(torch.int32), torch.zeros(1, dtype=torch.int32, device=dev)])
    return off, items


@dataclass
class Enriched:
    """What a metric keeps of one (recommendations, ground truth, k) call: the per-user values of every cut-off, on the
    device, and their deterministic sums."""
    users: torch.Tensor                  # [n] int64 ascending: the evaluated users
    ks: List[int]
    per_user: Optional[torch.Tensor]     # [n x n_ks] float64, None for Coverage
    sums: np.ndarray                     # [n_ks]
    means: Optional[Dict[int, float]] = None       # Coverage: the value itself
    counts: Optional[Dict[int, int]] = None        # Coverage: the numerators

    @property
    def n(self) -> int:
        return int(self.users.numel())


def _unpack(k, res: Dict[int, float]):
    if isinstance(k, (int, np.integer)):
        return res[int(k)]
    return {int(x): res[int(x)] for x in k}


class Metric:
    """Quality metric: metric(recommendations, ground_truth, k, ground_truth_users=None)
    (replay/metrics/base_metric.py:178-201).  Users: those of the ground truth, or `ground_truth_users`; a user without
    recommendations has an empty list and counts in the denominator."""

    _TOPK_INDEX: Optional[int] = None    # position in METRICS
    _EXTRA_INDEX: Optional[int] = None   # position in EXTRAS

    def __str__(self):
        return type(self).__name__

    # ---- the three stages of the reference: enrich, per-user distribution, aggregate -------------------------------
    def _user_set(self, rec, gt, ground_truth_users, dev) -> torch.Tensor:
        if ground_truth_users is not None:
            return _users(ground_truth_users, dev)
        return torch.unique(gt["user_idx"].to(torch.int64))

    def _enrich(self, recommendations, ground_truth, k, ground_truth_users=None) -> Enriched:
        dev = _device()
        ks = _ks_list(k)
        rec = _columns(recommendations, dev, need_rel=True)
        gt = _columns(ground_truth, dev)
        users = self._user_set(rec, gt, ground_truth_users, dev)
        n = int(users.numel())
        if n == 0:
            return Enriched(users, ks, torch.zeros((0, len(ks)), dtype=torch.float64, device=dev), np.zeros(len(ks)))
        g_off, g_items = _gt_csr(gt, users)
        per_user, sums = self._values(rec, users, ks, g_off, g_items, dev)
        return Enriched(users, ks, per_user, sums)

    def _values(self, rec, users, ks, g_off, g_items, dev):
        n = int(users.numel())
        block, _, _, _ = frame_to_block(_rows_of(users, rec["user_idx"]), rec["item_idx"], rec["relevance"], n, ks[-1])
        if self._TOPK_INDEX is not None:
            sums, pu = _eval_topk_sums(block, g_off, g_items, ks, None, True)
            return pu[:, self._TOPK_INDEX, :].contiguous(), sums[self._TOPK_INDEX]
        sums, pu = evaluate_extras(block, ks, g_off, g_items)
        return pu[:, self._EXTRA_INDEX, :].contiguous(), sums[self._EXTRA_INDEX]

    def _mean(self, enr: Enriched, k):
        res = {kk: (float(enr.sums[i]) / enr.n if enr.n else float("nan")) for i, kk in enumerate(enr.ks)}
        return _unpack(k, res)

    def _median(self, enr: Enriched, k):
        """The lower median, sorted[ceil(n / 2) - 1]: what percentile_approx(value, 0.5) (base_metric.py:229-238)
        returns while the data fit its accuracy."""
        res = {}
        for i, kk in enumerate(enr.ks):
            if enr.n == 0:
                res[kk] = float("nan")
                continue
            v = torch.sort(enr.per_user[:, i]).values
            res[kk] = float(v[math.ceil(enr.n / 2) - 1])
        return _unpack(k, res)

    def _conf_interval(self, enr: Enriched, k, alpha: float = 0.95):
        """norm.ppf((1 + alpha) / 2) * stddev (sample, cast to float as base_metric.py:203-227 does) / sqrt(count)."""
        q = NormalDist().inv_cdf((1 + alpha) / 2)
        res = {}
        for i, kk in enumerate(enr.ks):
            std = float(torch.std(enr.per_user[:, i], unbiased=True)) if enr.n > 1 else float("nan")
            std = 0.0 if math.isnan(std) else float(np.float32(std))
            res[kk] = q * std / math.sqrt(enr.n) if enr.n else 0.0
        return _unpack(k, res)

    def __call__(self, recommendations, ground_truth, k, ground_truth_users=None):
        return self._mean(self._enrich(recommendations, ground_truth, k, ground_truth_users), k)

    def median(self, recommendations, ground_truth, k, ground_truth_users=None):
        return self._median(self._enrich(recommendations, ground_truth, k, ground_truth_users), k)

    def conf_interval(self, recommendations, ground_truth, k, alpha: float = 0.95, ground_truth_users=None):
        return self._conf_interval(self._enrich(recommendations, ground_truth, k, ground_truth_users), k, alpha)

    def user_distribution(self, log, recommendations, ground_truth, k, ground_truth_users=None):
        """Mean value over the users with the same number of rows in `log` (base_metric.py:281-334): a pandas frame
        [count, value] ordered by count, one group of rows per cut-off; users the log does not hold have count 0."""
        import pandas as pd
        enr = self._enrich(recommendations, ground_truth, k, ground_truth_users)
        lg = _columns(log, enr.users.device)
        rows = _rows_of(enr.users, lg["user_idx"]).to(torch.int64)
        count = torch.bincount(rows[rows >= 0], minlength=enr.n).cpu().numpy()
        ks = [int(k)] if isinstance(k, (int, np.integer)) else [int(x) for x in k]
        parts = []
        for kk in ks:
            v = enr.per_user[:, enr.ks.index(kk)].cpu().numpy()
            parts.append(pd.DataFrame({"count": count, "value": v}).groupby("count", as_index=False)["value"].mean()
                         .sort_values("count"))
        return pd.concat(parts, ignore_index=True) if parts else pd.DataFrame({"count": [], "value": []})


class NDCG(Metric):
    _TOPK_INDEX = 0


class HitRate(Metric):
    _TOPK_INDEX = 1


class Precision(Metric):
    _TOPK_INDEX = 2


class Recall(Metric):
    _TOPK_INDEX = 3


class MAP(Metric):
    _TOPK_INDEX = 4


class MRR(Metric):
    _TOPK_INDEX = 5


class RocAuc(Metric):
    _EXTRA_INDEX = 0


class NCISPrecision(Metric):
    """Precision with normalised capped importance-sampling weights (replay/metrics/base_metric.py:391-588,
    ncis_precision.py).  `prev_policy_weights`: [user_idx,] item_idx, relevance of the previous policy; where it holds
    a key more than once, the first relevance in (key, relevance) order is taken."""
    _EXTRA_INDEX = 3

    def __init__(self, prev_policy_weights, threshold: float = 10.0, activation: Optional[str] = None):
        if activation not in _ACTIVATIONS:
            raise ValueError(f"Unexpected `activation` - {activation}")
        if threshold <= 0:
            raise ValueError("Threshold should be positive real number")
        dev = _device()
        self.threshold, self.activation = float(threshold), activation
        prev = _columns(prev_policy_weights, dev, need_rel=True, need_user=False)
        self._by_user = prev["user_idx"] is not None
        key = prev["item_idx"].to(torch.int64) & 0xFFFFFFFF
        if self._by_user:
            key = key | ((prev["user_idx"].to(torch.int64) & 0xFFFFFFFF) << 32)
        # ascending as UNSIGNED 64-bit keys: ids are non-negative int32, so the signed order is the same
        if key.numel() and (int(prev["item_idx"].min()) < 0 or (self._by_user and int(prev["user_idx"].min()) < 0)):
            raise ValueError("prev_policy_weights: ids must be non-negative")
        order = torch.argsort(key, stable=True)
        self._keys, self._vals = key[order].contiguous(), prev["relevance"][order].contiguous()

    def _values(self, rec, users, ks, g_off, g_items, dev):
        eng = Engine(dev)
        n, kmax = int(users.numel()), ks[-1]
        n_rows = int(rec["item_idx"].numel())
        prev = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        if n_rows:
            if self._by_user and int(rec["user_idx"].min()) < 0:
                raise ValueError("user_idx must be non-negative")
            eng.call("recs_join_prev", self._keys, self._vals, int(self._keys.numel()),
                     rec["user_idx"] if self._by_user else None, rec["item_idx"], n_rows, prev)
        block, val, _, w = frame_to_block(_rows_of(users, rec["user_idx"]), rec["item_idx"], rec["relevance"], n, kmax,
                                          dedup=False, payload=prev, want_val=True)
        eng.call("recs_ncis_weights", block, val, w, n, kmax, _ACTIVATIONS[self.activation], self.threshold)
        self._last_block = (block, val, w)       # the enriched lists, for inspection
        sums, pu = evaluate_extras(block, ks, g_off, g_items, rec_w=w)
        return pu[:, self._EXTRA_INDEX, :].contiguous(), sums[self._EXTRA_INDEX]


class RecOnlyMetric(Metric):
    """metric(recommendations, k, ground_truth_users=None) (replay/metrics/base_metric.py:338-388)."""

    def __call__(self, recommendations, k, ground_truth_users=None):      # pylint: disable=arguments-differ
        return self._mean(self._enrich(recommendations, None, k, ground_truth_users), k)

    def median(self, recommendations, k, ground_truth_users=None):        # pylint: disable=arguments-differ
        return self._median(self._enrich(recommendations, None, k, ground_truth_users), k)

    def conf_interval(self, recommendations, k, alpha: float = 0.95, ground_truth_users=None):  # pylint: disable=arguments-differ
        return self._conf_interval(self._enrich(recommendations, None, k, ground_truth_users), k, alpha)

    def user_distribution(self, log, recommendations, ground_truth, k, ground_truth_users=None):
        raise NotImplementedError("user_distribution is defined for the metrics that take a ground truth")


class Surprisal(RecOnlyMetric):
    """Mean normalised self-information of the recommended items (replay/metrics/surprisal.py).  Users: those of the
    recommendations, or `ground_truth_users`."""

    def __init__(self, log):
        dev = _device()
        lg = _columns(log, dev)
        if lg["item_idx"].numel() and int(lg["item_idx"].min()) < 0:
            raise ValueError("item_idx must be non-negative")
        self.item_weights = surprisal_weights(lg["item_idx"], lg["user_idx"])

    def _enrich(self, recommendations, ground_truth, k, ground_truth_users=None) -> Enriched:
        dev = _device()
        ks = _ks_list(k)
        rec = _columns(recommendations, dev, need_rel=True)
        users = _users(ground_truth_users, dev) if ground_truth_users is not None else \
            torch.unique(rec["user_idx"].to(torch.int64))
        n = int(users.numel())
        if n == 0:
            return Enriched(users, ks, torch.zeros((0, len(ks)), dtype=torch.float64, device=dev), np.zeros(len(ks)))
        block, _, _, _ = frame_to_block(_rows_of(users, rec["user_idx"]), rec["item_idx"], rec["relevance"], n, ks[-1])
        sums, pu = evaluate_extras(block, ks, item_w=self.item_weights)
        return Enriched(users, ks, pu[:, 2, :].contiguous(), sums[2])


class Unexpectedness(RecOnlyMetric):
    """1 - |pred[:k] & base[:k]| / k against the predictions of a base model (replay/metrics/unexpectedness.py).
    Users: those of the base predictions, or `ground_truth_users`; the base list is the user's whole base frame with
    repeats dropped, up to MAX_BASE rows of it."""
    MAX_BASE = 1024

    def __init__(self, pred):
        self._base = _columns(pred, _device(), need_rel=True)

    def _enrich(self, recommendations, ground_truth, k, ground_truth_users=None) -> Enriched:
        dev = _device()
        ks = _ks_list(k)
        rec = _columns(recommendations, dev, need_rel=True)
        base = self._base
        base_users = torch.unique(base["user_idx"].to(torch.int64))
        users = _users(ground_truth_users, dev) if ground_truth_users is not None else base_users
        n = int(users.numel())
        if n == 0:
            return Enriched(users, ks, torch.zeros((0, len(ks)), dtype=torch.float64, device=dev), np.zeros(len(ks)))
        # the recommendations are right-joined to the base lists first (:77-86): a user without one has no list at all
        rows = _rows_of(users, rec["user_idx"])
        rows = torch.where(_rows_of(base_users, rec["user_idx"]) >= 0, rows, torch.full_like(rows, -1))
        block, _, _, _ = frame_to_block(rows, rec["item_idx"], rec["relevance"], n, ks[-1])
        brows = _rows_of(users, base["user_idx"])
        longest = int(torch.bincount(brows[brows >= 0].to(torch.int64), minlength=1).max()) if brows.numel() else 0
        kb = max(ks[-1], min(longest, self.MAX_BASE))
        bblock, _, _, _ = frame_to_block(brows, base["item_idx"], base["relevance"], n, kb)
        sums, pu = evaluate_extras(block, ks, base_idx=bblock)
        return Enriched(users, ks, pu[:, 1, :].contiguous(), sums[1])


class Coverage(RecOnlyMetric):
    """Share of the log's items that reach some user's top k (replay/metrics/coverage.py).  Not averaged over users;
    items the log does not hold count in the numerator, so the value can exceed 1."""

    def __init__(self, log):
        dev = _device()
        self.item_count = int(torch.unique(_columns(log, dev, need_user=False)["item_idx"]).numel())

    def _enrich(self, recommendations, ground_truth, k, ground_truth_users=None) -> Enriched:
        dev = _device()
        ks = _ks_list(k)
        rec = _columns(recommendations, dev, need_rel=True)
        users = torch.unique(rec["user_idx"].to(torch.int64))
        if ground_truth_users is not None:                      # inner join (:48-52)
            users = users[torch.isin(users, _users(ground_truth_users, dev))]
        n = int(users.numel())
        counts = [0] * len(ks)
        if n:
            block, _, pos, _ = frame_to_block(_rows_of(users, rec["user_idx"]), rec["item_idx"], rec["relevance"], n,
                                              ks[-1], want_pos=True)
            counts = coverage_counts(block, pos, ks)
        means = {kk: c / self.item_count for kk, c in zip(ks, counts)}
        return Enriched(users, ks, None, np.array([means[kk] for kk in ks]), means, dict(zip(ks, counts)))

    def _mean(self, enr: Enriched, k):
        return _unpack(k, enr.means)

    def _median(self, enr: Enriched, k):
        return self._mean(enr, k)

    def _conf_interval(self, enr: Enriched, k, alpha: float = 0.95):
        return _unpack(k, {kk: 0.0 for kk in enr.ks})

    def numerators(self, recommendations, k, ground_truth_users=None):
        """The integer numerators: items with a best position <= k."""
        return _unpack(k, self._enrich(recommendations, None, k, ground_truth_users).counts)


def item_distribution(log, recommendations, k: int):
    """Item popularity in `log` and in the top-k `recommendations` (replay/distributions.py:62-94): a pandas frame
    [item_idx, user_count, rec_count] ordered by (user_count, item_idx); both counts are numbers of distinct users."""
    import pandas as pd
    dev = _device()
    lg = _columns(log, dev)
    rec = _columns(recommendations, dev, need_rel=True)
    for c in (lg, rec):
        if c["item_idx"].numel() and int(c["item_idx"].min()) < 0:
            raise ValueError("item_idx must be non-negative")
    n_items = max([int(c["item_idx"].max()) + 1 for c in (lg, rec) if c["item_idx"].numel()], default=0)
    if n_items == 0:
        return pd.DataFrame({"item_idx": [], "user_count": [], "rec_count": []})
    user_count, _ = item_user_counts(lg["item_idx"], lg["user_idx"], n_items)
    rec_count = torch.zeros(n_items, dtype=torch.int32, device=dev)
    users = torch.unique(rec["user_idx"].to(torch.int64))
    if users.numel():
        # distinct users per item within the top k rows: a block cut at k with repeats dropped holds an item once per user
        block, _, _, _ = frame_to_block(_rows_of(users, rec["user_idx"]), rec["item_idx"], rec["relevance"],
                                        int(users.numel()), int(k))
        Engine(dev).call("eval_item_hist", block, int(users.numel()), int(k), n_items, rec_count)
    present = torch.nonzero((user_count > 0) | (rec_count > 0)).flatten()
    uc, rc = user_count[present].to(torch.int64), rec_count[present].to(torch.int64)
    order = torch.argsort(uc * n_items + present, stable=True)
    return pd.DataFrame({"item_idx": present[order].cpu().numpy(), "user_count": uc[order].cpu().numpy(),
                         "rec_count": rc[order].cpu().numpy()})
