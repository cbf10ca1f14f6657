"""Times the device filters and the Indexer (replay_cql_amd.filters / .indexer -> csrc/prepare.hip) on the cfg3 log and,
beside them in the same process, a pandas implementation of the same steps on the same log.

    python tools/prepare_bench.py [--users 1000000] [--repeats 5] [--pandas-repeats 2] [--out profiles/prepare_bench.json]

The log is data.synth_log_device's (1 M users, 100 000 items, about 48 M rows), generated on the device and flattened
to LOG_SCHEMA columns in a fixed random row order, as tools/split_bench.py makes it.  Its timestamp is unique inside a
user, so the last-N filter does not depend on a tie-break and both paths must return the SAME rows -- which is checked.
For the Indexer the ids are made sparse: raw id = data._mix64(dense id), any int64, negative ones among them.

Timed: filter_out_low_ratings(0.5), filter_by_min_count(40) on users, filter_by_min_count(400, "item_idx"),
take_num_user_interactions(20, first=False), Indexer.fit + transform.
  device   the whole call on the dict of device columns, device columns out (host clock around the call, which ends in
           the compaction's device-to-host read of the length plus a synchronise after the gathers)
  pandas   boolean masks from groupby / transform / rank on a host DataFrame of the same columns, then the frame; the
           Indexer as numpy unique + searchsorted on both id columns (host clock)
One warm-up of every device call, then `repeats` device runs and `pandas-repeats` pandas runs; median and spread
(max - min) of each.  Needs a GPU."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.bench_record import make_log, spread          # noqa: E402  pylint: disable=wrong-import-position


# ---- the pandas side: the keep mask of each filter -------------------------------------------------------------
def pandas_low_ratings(df):
    return (df["relevance"] >= 0.5).to_numpy()


def pandas_min_count_users(df):
    return (df.groupby("user_idx")["user_idx"].transform("count") >= 40).to_numpy()


def pandas_min_count_items(df):
    return (df.groupby("item_idx")["item_idx"].transform("count") >= 400).to_numpy()


def pandas_last_20(df):
    # (timestamp, item, row) descending inside the user: the timestamp is unique inside a user, so rank needs no more
    return (df.groupby("user_idx")["timestamp"].rank(method="first", ascending=False) <= 20).to_numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pandas-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_bench needs a GPU: a CPU run gives no time")
    import pandas as pd
    from replay_cql_amd import data as D
    from replay_cql_amd import filters as F
    from replay_cql_amd.indexer import Indexer
    dev = torch.device("cuda:0")
    log = make_log(args.users, args.items, dev)
    n_rows = int(log["user_idx"].numel())
    frame = pd.DataFrame({k: v.cpu().numpy() for k, v in log.items()})
    cases = [("filter_out_low_ratings(0.5)", lambda x, **kw: F.filter_out_low_ratings(x, 0.5, **kw), pandas_low_ratings),
             ("filter_by_min_count(40, user_idx)", lambda x, **kw: F.filter_by_min_count(x, 40, **kw), pandas_min_count_users),
             ("filter_by_min_count(400, item_idx)", lambda x, **kw: F.filter_by_min_count(x, 400, "item_idx", **kw),
              pandas_min_count_items),
             ("take_num_user_interactions(20, first=False)",
              lambda x, **kw: F.take_num_user_interactions(x, 20, first=False, **kw), pandas_last_20)]
    result = {"device": torch.cuda.get_device_name(0), "users": args.users, "items": args.items, "rows": n_rows,
              "repeats": args.repeats, "pandas_repeats": args.pandas_repeats, "calls": {}}

    def timed(fn, sync):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def record(name, t_dev, t_pd, same, **more):
        row = {"device_s": t_dev, "pandas_s": t_pd, "device_median_s": statistics.median(t_dev),
               "pandas_median_s": statistics.median(t_pd), "device_spread_s": spread(t_dev), "pandas_spread_s": spread(t_pd),
               "rows_per_s_device": n_rows / statistics.median(t_dev), "same_rows_as_pandas": same,
               "pandas_over_device": statistics.median(t_pd) / statistics.median(t_dev), **more}
        result["calls"][name] = row
        print(json.dumps({"call": name, **{k: v for k, v in row.items() if k not in ("device_s", "pandas_s")}}), flush=True)
        if not same:
            raise SystemExit(f"{name}: the device path and pandas return different rows")

    for name, call, fn in cases:
        timed(lambda: call(log), True)                                    # warm-up: code objects, rocPRIM's choices
        t_dev = [timed(lambda: call(log), True)[0] for _ in range(args.repeats)]
        rows = call(log, return_rows=True).cpu().numpy()
        def pandas_run():
            mask = fn(frame)
            return mask, frame[mask]

        t_pd, mask = [], None
        for _ in range(args.pandas_repeats):
            t, (mask, _) = timed(pandas_run, False)
            t_pd.append(t)
        record(name, t_dev, t_pd, bool(np.array_equal(rows, np.flatnonzero(mask))), kept_rows=int(len(rows)))

    # the Indexer on sparse raw ids
    raw = {"user_id": D._mix64(log["user_idx"].to(torch.int64)), "item_id": D._mix64(log["item_idx"].to(torch.int64) + (1 << 40)),
           "timestamp": log["timestamp"], "relevance": log["relevance"]}
    raw_frame = pd.DataFrame({k: v.cpu().numpy() for k, v in raw.items()})

    def device_index():
        ix = Indexer()
        ix.fit(raw, raw)
        return ix, ix.transform(raw)

    def pandas_index():
        out = {}
        for col, idx in (("user_id", "user_idx"), ("item_id", "item_idx")):
            ids = raw_frame[col].to_numpy()
            labels = np.unique(ids)
            out[idx] = np.searchsorted(labels, ids).astype(np.int32)
        return raw_frame.drop(columns=["user_id", "item_id"]).assign(**out)

    timed(device_index, True)
    t_dev = [timed(device_index, True)[0] for _ in range(args.repeats)]
    ix, got = device_index()
    t_pd, want = [], None
    for _ in range(args.pandas_repeats):
        t, want = timed(pandas_index, False)
        t_pd.append(t)
    same = bool(np.array_equal(got["user_idx"].cpu().numpy(), want["user_idx"].to_numpy()) and
                np.array_equal(got["item_idx"].cpu().numpy(), want["item_idx"].to_numpy()))
    record("Indexer.fit + transform", t_dev, t_pd, same, user_labels=int(ix.user_labels.numel()),
           item_labels=int(ix.item_labels.numel()))
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
