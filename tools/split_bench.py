"""Times the device splitters (replay_cql_amd.splitters -> csrc/split.hip) on the cfg3 log and, beside them in the same
process, a pandas implementation of the same splits on the same log.

    python tools/split_bench.py [--users 1000000] [--repeats 5] [--pandas-repeats 2] [--out profiles/split_bench.json]

The log is data.synth_log_device's (1 M users, 100 000 items, about 48 M rows), generated on the device and flattened
to LOG_SCHEMA columns in a fixed random row order.  Its timestamp is the position inside the user plus a per-user start
(a hash of the user id, 0..999): unique inside a user, so the splits do not depend on a tie-break and both paths must
return the SAME rows -- which is checked -- while users start at different dates, so NewUsersSplitter has something to cut.

Timed: UserSplitter(item_test_size=1, drop_cold_items=True), DateSplitter(0.2), NewUsersSplitter(0.1).
  device   split() on the dict of device columns: both parts come back as device columns (host clock around the call,
           which ends in the compaction's device-to-host read of the two lengths plus a synchronise after the gathers)
  pandas   boolean masks from groupby / rank / isin on a host DataFrame of the same columns, then the two frames
           (host clock)
One warm-up of every device split, then `repeats` device runs and `pandas-repeats` pandas runs; median and spread
(max - min) of each.  The pandas runs dominate the wall time, so they are few.  Needs a GPU."""
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


# ---- the pandas side: (train mask, test mask) of each split -----------------------------------------------------
def pandas_user_last(df):
    rank = df.groupby("user_idx")["timestamp"].rank(method="first", ascending=False)
    test = (rank <= 1).to_numpy()
    train = ~test
    test &= df["item_idx"].isin(df["item_idx"].to_numpy()[train]).to_numpy()
    test &= (df["relevance"] > 0.0).to_numpy()
    return train, test


def pandas_date(df, frac=0.2):
    ts = df["timestamp"].to_numpy()
    m = int(len(ts) * (1 - frac)) + 1
    thr = np.partition(ts, m - 1)[m - 1]
    test = ts >= thr
    return ~test, test & (df["relevance"] > 0.0).to_numpy()


def pandas_new_users(df, test_size=0.1):
    start = df.groupby("user_idx")["timestamp"].transform("min").to_numpy()
    starts = df.groupby("user_idx")["timestamp"].min()
    by_date = starts.value_counts().sort_index(ascending=False).cumsum()
    thr = by_date[by_date >= len(starts) * test_size].index.max()
    ts = df["timestamp"].to_numpy()
    return ts < thr, (start >= thr) & (df["relevance"] > 0.0).to_numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pandas-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("split_bench needs a GPU: a CPU run gives no time")
    import pandas as pd
    from replay_cql_amd import splitters as S
    dev = torch.device("cuda:0")
    log = make_log(args.users, args.items, dev)
    n_rows = int(log["user_idx"].numel())
    frame = pd.DataFrame({k: v.cpu().numpy() for k, v in log.items()})
    cases = [("UserSplitter(item_test_size=1, drop_cold_items=True)", S.UserSplitter(item_test_size=1, drop_cold_items=True),
              pandas_user_last),
             ("DateSplitter(0.2)", S.DateSplitter(0.2), pandas_date),
             ("NewUsersSplitter(0.1)", S.NewUsersSplitter(0.1), pandas_new_users)]
    result = {"device": torch.cuda.get_device_name(0), "users": args.users, "items": args.items, "rows": n_rows,
              "repeats": args.repeats, "pandas_repeats": args.pandas_repeats, "splits": {}}

    def device_run(splitter):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train, test = splitter.split(log)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, train, test

    def pandas_run(fn):
        t0 = time.perf_counter()
        train, test = fn(frame)
        parts = frame[train], frame[test]
        return time.perf_counter() - t0, train, test, parts

    for name, splitter, fn in cases:
        device_run(splitter)                                              # warm-up: code objects, rocPRIM's choices
        t_dev, t_pd = [], []
        for _ in range(args.repeats):
            t, train, test = device_run(splitter)
            t_dev.append(t)
        rows = [x.cpu().numpy() for x in splitter.split_indices(log)]
        del train, test
        for _ in range(args.pandas_repeats):
            t, m_train, m_test, _ = pandas_run(fn)
            t_pd.append(t)
        same = bool(np.array_equal(rows[0], np.flatnonzero(m_train)) and np.array_equal(rows[1], np.flatnonzero(m_test)))
        row = {"device_s": t_dev, "pandas_s": t_pd, "device_median_s": statistics.median(t_dev),
               "pandas_median_s": statistics.median(t_pd), "device_spread_s": spread(t_dev), "pandas_spread_s": spread(t_pd),
               "rows_per_s_device": n_rows / statistics.median(t_dev), "train_rows": int(len(rows[0])),
               "test_rows": int(len(rows[1])), "same_rows_as_pandas": same,
               "pandas_over_device": statistics.median(t_pd) / statistics.median(t_dev)}
        result["splits"][name] = row
        print(json.dumps({"split": name, **{k: v for k, v in row.items() if k not in ("device_s", "pandas_s")}}), flush=True)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
