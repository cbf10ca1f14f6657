"""The log, whatever kind it came as: `_Log` gives the columns of a pandas frame, a pyarrow
table / batch or a dict of device tensors as device tensors and `take(rows)` back as the kind that came in; the functions
beside it look at a log's columns without a GPU and range-check its ids."""
from __future__ import annotations

import numpy as np
import torch

from . import data as D

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


class _Log:
    """Columns of a log as device tensors (made on demand) + `take(rows)` that gives back the kind that came in."""

    def __init__(self, log):
        self.kind, self.src = None, log
        try:
            import pandas as pd
            if isinstance(log, pd.DataFrame):
                self.kind, self.n, self.names = "pandas", len(log), list(log.columns)
        except ImportError:  # pragma: no cover
            pass
        if self.kind is None and isinstance(log, dict):
            tens = [v for v in log.values() if torch.is_tensor(v)]
            if not tens:
                raise ValueError("a dict log must hold device tensors")
            self.kind, self.n, self.names = "device", int(tens[0].shape[0]), list(log.keys())
            self.device = tens[0].device
            if any(t.shape[0] != self.n or t.device != self.device for t in tens):
                raise ValueError("log columns differ in length or device")
        if self.kind is None:
            import pyarrow as pa
            if isinstance(log, pa.RecordBatch):
                self.kind, self.table = "batch", pa.Table.from_batches([log])
            elif isinstance(log, pa.Table):
                self.kind, self.table = "table", log
            else:
                batches = list(log)
                if not batches or not all(isinstance(b, pa.RecordBatch) for b in batches):
                    raise ValueError(f"cannot split a log of type {type(log)}: pandas, pyarrow or a dict of tensors")
                self.kind, self.table = "table", pa.Table.from_batches(batches)
            self.n, self.names = self.table.num_rows, list(self.table.schema.names)
        if self.kind != "device":
            if not torch.cuda.is_available():
                from ._native import CqlrecError
                raise CqlrecError("split() needs a GPU: the splitters have no CPU path")
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ts_kind = None

    def _host(self, name: str) -> np.ndarray:
        if name not in self.names:
            raise ValueError(f"log has no column {name}")
        if self.kind == "pandas":
            return self.src[name].to_numpy()
        col = self.table.column(name)
        if col.null_count:
            raise ValueError(f"column {name} contains nulls")
        return col.combine_chunks().to_numpy(zero_copy_only=False)

    def ids(self, name: str):
        if self.kind == "device":
            if name not in self.names:
                raise ValueError(f"log has no column {name}")
            t = self.src[name]
            if t.dtype.is_floating_point:
                raise ValueError(f"column {name} must be an integer column")
            return t.to(torch.int64).contiguous()         # narrowed after the range check
        a = self._host(name)
        if a.dtype.kind not in "iu":
            raise ValueError(f"column {name} must be an integer column, got {a.dtype}")
        return D._dev_col(a.astype(np.int64, copy=False), torch.int64, self.device)

    def key(self, name: str):
        """timestamp_key of the column `name` as an int64 device tensor; sets ts_kind (datetime / int / float)."""
        if self.kind == "device":
            if name not in self.names:
                raise ValueError(f"log has no column {name}")
            t = self.src[name]
            self.ts_kind = "float" if t.dtype.is_floating_point else "int"
            return D.timestamp_key(t).contiguous()
        a = self._host(name)
        self.ts_kind = {"M": "datetime", "i": "int", "u": "int", "f": "float"}.get(a.dtype.kind)
        if self.ts_kind is None:
            raise ValueError(f"column {name} has unsupported dtype {a.dtype}")
        return D._dev_col(D.timestamp_key(a), torch.int64, self.device)

    def take(self, rows):
        if self.kind == "device":
            return {k: (v[rows] if torch.is_tensor(v) else v) for k, v in self.src.items()}
        idx = rows.cpu().numpy()
        if self.kind == "pandas":
            return self.src.iloc[idx].reset_index(drop=True)
        import pyarrow as pa
        out = self.table.take(pa.array(idx))
        if self.kind == "batch":
            out = out.combine_chunks()
            return out.to_batches()[0] if out.num_rows else pa.RecordBatch.from_pylist([], schema=out.schema)
        return out


def open_log(log, what: str) -> _Log:
    """_Log of a normalised log, on a GPU: CqlrecError without one, ValueError beyond 2^31 - 1 rows."""
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
    """the column `name` as a float64 device tensor"""
    if lg.kind == "device":
        return lg.src[name].to(torch.float64).contiguous()
    return D._dev_col(lg._host(name).astype(np.float64, copy=False), torch.float64, lg.device)


def dense_ids(lg: _Log, names, label: str = ""):
    """[(int32 device ids, largest id + 1)] of the integer columns `names`, range-checked in one small sync: the kernels
    index count arrays and bitmaps with them.  `label` names the columns in the errors (default: their own names)."""
    label = label or " / ".join(names)
    cols = [lg.ids(nm) for nm in names]
    lim = torch.stack([f(c) for c in cols for f in (torch.min, torch.max)]).cpu().tolist()
    if min(lim[0::2]) < 0:
        raise ValueError(f"{label} must be non-negative dense indices")
    if max(lim[1::2]) >= (1 << 31) - 1:
        raise ValueError(f"{label} must be below 2^31 - 1")
    return [(c.to(torch.int32), int(hi) + 1) for c, hi in zip(cols, lim[1::2])]
