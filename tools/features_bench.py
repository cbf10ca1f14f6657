"""Times the history-based feature processors (replay_cql_amd.history_based_fp -> csrc/features.hip) on the cfg3 log
and, beside them in the same process, a pandas implementation of the same fit and the torch composition of the block.

    python tools/features_bench.py [--users 1000000] [--candidates 100] [--repeats 5] [--pandas-repeats 1]
                                   [--out profiles/features_bench.json]

The log is tools/bench_record.make_log's (1 M users, 100 000 items, about 48 M rows, device columns in, fixed random row
order); its timestamp (start + position inside the user) is taken as HOURS, so that a user's history spans days.  The
categorical features are user_idx % 7 and item_idx % 13, listed for every id.

Timed, each as the median of `repeats` whole calls after one warm-up (host clock around a call that ends in a device
synchronise), with the spread (max - min):
  LogStatFeaturesProcessor.fit                  pandas: groupby aggregations for the same columns of both tables
  HistoryBasedFeaturesProcessor.fit             one user and one item categorical column; pandas: the same plus the two
                                                (entity, category) count tables
  transform_block, users x candidates, float32  torch: index_select per table, where, searchsorted, cat -- on float32
                                                copies of the tables made outside the timed window
For the block the bytes written (n_pairs * F * 4) over the time are reported, next to the rate of a plain fill of a
tensor of the block's size in the same process (a write-only yardstick) and, when --hbm-json names the output of
tools/hbm_microbench.py --modes adam, that tool's streaming rate.  Needs a GPU."""
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

DAY_S = 86400


# ---- the pandas side ---------------------------------------------------------------------------------------------
def pandas_log_stat(df):
    """user and item tables with the columns LogStatFeaturesProcessor fits (quantiles by pandas' `higher` rule)"""
    import pandas as pd
    day = df["timestamp"] // DAY_S
    last_day = int(df["timestamp"].max()) // DAY_S
    tabs = {}
    for pre, col in (("u", "user_idx"), ("i", "item_idx")):
        g = df.groupby(col, sort=True)
        rel = g["relevance"].agg(["count", "mean", "std"])
        q = g["relevance"].quantile([0.05, 0.5, 0.95], interpolation="higher").unstack()
        ts = g["timestamp"].agg(["min", "max"])
        days = day.groupby(df[col], sort=True).nunique()
        tabs[pre] = pd.DataFrame({
            f"{pre}_log_num_interact": np.log(rel["count"]), f"{pre}_log_interact_days_count": np.log(days),
            f"{pre}_min_interact_date": ts["min"], f"{pre}_max_interact_date": ts["max"],
            f"{pre}_std": rel["std"].fillna(0.0), f"{pre}_mean": rel["mean"], f"{pre}_quantile_05": q[0.05],
            f"{pre}_quantile_5": q[0.5], f"{pre}_quantile_95": q[0.95],
            f"{pre}_history_length_days": ts["max"] // DAY_S - ts["min"] // DAY_S,
            f"{pre}_last_interaction_gap_days": last_day - ts["max"] // DAY_S})

    def dense(series, n):
        out = np.zeros(n)
        out[series.index.to_numpy()] = series.to_numpy()
        return out
    user, item = df["user_idx"].to_numpy(), df["item_idx"].to_numpy()
    n_users, n_items = int(user.max()) + 1, int(item.max()) + 1
    i_mean, i_std = dense(tabs["i"]["i_mean"], n_items), dense(tabs["i"]["i_std"], n_items)
    ab = np.abs(df["relevance"].to_numpy() - i_mean[item])
    lo, hi = tabs["i"]["i_std"].min(), tabs["i"]["i_std"].max()
    by_user = pd.DataFrame({"user_idx": user, "abnormality": ab,
                            "abnormalityCR": (ab * (1.0 - (i_std[item] - lo) / (hi - lo))) ** 2,
                            "u_mean_i_log_num_interact": dense(tabs["i"]["i_log_num_interact"], n_items)[item]})
    tabs["u"] = tabs["u"].join(by_user.groupby("user_idx", sort=True).mean())
    cross = pd.Series(dense(tabs["u"]["u_log_num_interact"], n_users)[user]).groupby(item, sort=True).mean()
    tabs["i"]["i_mean_u_log_num_interact"] = cross
    return tabs


def pandas_cond_pop(df, features, col):
    join_col, entity = ("item_idx", "user_idx") if "item_idx" in features.columns else ("user_idx", "item_idx")
    cat = features.set_index(join_col)[col].reindex(df[join_col].to_numpy()).to_numpy()
    counts = df.groupby([df[entity].to_numpy(), cat], sort=True, dropna=False).size()
    total = df.groupby(entity, sort=True).size()
    return counts / total.reindex(counts.index.get_level_values(0)).to_numpy()


# ---- the torch composition of the block ------------------------------------------------------------------------
def torch_block(fp, user, item, tabs32):
    log, out = fp.log_processor, []
    cold = {}
    for pre, ids, count, tab in (("u", user, log._ucount, tabs32[0]), ("i", item, log._icount, tabs32[1])):
        inside = (ids >= 0) & (ids < count.numel())
        safe = torch.where(inside, ids, torch.zeros_like(ids))
        cold[pre] = ~inside | (count.index_select(0, safe) == 0)
        out.append(torch.where(cold[pre].unsqueeze(1), 0.0, tab.index_select(0, safe)))
    u_at, i_at = log._unames.index, log._inames.index
    extra = [cold["u"].to(torch.float32), cold["i"].to(torch.float32),
             out[0][:, u_at("u_log_num_interact")] - out[1][:, i_at("i_mean_u_log_num_interact")],
             out[1][:, i_at("i_log_num_interact")] - out[0][:, u_at("u_mean_i_log_num_interact")]]
    for proc in (fp.user_cond_pop_proc, fp.item_cond_pop_proc):
        for col in proc.conditional_pop_dict:
            t = proc.conditional_pop_dict.table(col)
            e, o = (item, user) if t["entity_is_item"] else (user, item)
            known = (o >= 0) & (o < t["code"].numel())
            code = torch.where(known, t["code"][o.clamp(0, t["code"].numel() - 1)].to(torch.int64), t["n_cat"])
            key = e * (t["n_cat"] + 1) + code
            at = torch.searchsorted(t["keys"], key).clamp_(max=t["keys"].numel() - 1)
            hit = (t["keys"][at] == key) & (code < t["n_cat"])
            extra += [torch.where(hit, t["pop"][at], 0.0).to(torch.float32), (~hit).to(torch.float32)]
    return torch.cat(out + [torch.stack(extra, dim=1)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pandas-repeats", type=int, default=1)
    ap.add_argument("--hbm-json", default=None, help="a file holding the JSON line of tools/hbm_microbench.py --modes adam")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("features_bench needs a GPU: a CPU run gives no time")
    import pandas as pd
    from replay_cql_amd import history_based_fp as H
    dev = torch.device("cuda:0")
    log = make_log(args.users, args.items, dev)
    log["timestamp"] = log["timestamp"] * 3600
    n_rows = int(log["user_idx"].numel())
    user_features = pd.DataFrame({"user_idx": np.arange(args.users), "group": np.arange(args.users) % 7})
    item_features = pd.DataFrame({"item_idx": np.arange(args.items), "kind": np.arange(args.items) % 13})
    result = {"device": torch.cuda.get_device_name(0), "users": args.users, "items": args.items, "rows": n_rows,
              "repeats": args.repeats, "pandas_repeats": args.pandas_repeats, "calls": {}}

    def timed(fn, sync=True):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def record(name, t_dev, t_base, base, **more):
        row = {"device_s": t_dev, f"{base}_s": t_base, "device_median_s": statistics.median(t_dev),
               f"{base}_median_s": statistics.median(t_base), "device_spread_s": spread(t_dev),
               f"{base}_spread_s": spread(t_base), f"{base}_over_device": statistics.median(t_base) / statistics.median(t_dev),
               **more}
        result["calls"][name] = row
        print(json.dumps({"call": name, **{k: v for k, v in row.items() if not isinstance(v, list)}}), flush=True)
        if args.out:                                     # after every call: a later one running long loses nothing
            path = Path(args.out)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(result, indent=1) + "\n")

    def fit_log_stat():
        proc = H.LogStatFeaturesProcessor()
        proc.fit(log)
        return proc

    def fit_all():
        fp = H.HistoryBasedFeaturesProcessor(user_cat_features_list=["group"], item_cat_features_list=["kind"])
        fp.fit(log, user_features, item_features)
        return fp

    frame = pd.DataFrame({k: v.cpu().numpy() for k, v in log.items()})
    timed(fit_log_stat)
    t_dev = [timed(fit_log_stat)[0] for _ in range(args.repeats)]
    proc = fit_log_stat()
    t_pd, tabs = [], None
    for _ in range(args.pandas_repeats):
        t, tabs = timed(lambda: pandas_log_stat(frame), False)
        t_pd.append(t)
    got, want = proc.user_log_features, tabs["u"]
    agree = {c: float(np.max(np.abs(got[c].to_numpy().astype(np.float64) - want[c].to_numpy().astype(np.float64))))
             for c in ("u_log_num_interact", "u_mean", "u_std", "abnormality", "abnormalityCR", "u_mean_i_log_num_interact",
                       "u_history_length_days", "u_log_interact_days_count")}
    record("LogStatFeaturesProcessor.fit", t_dev, t_pd, "pandas", rows_per_s_device=n_rows / statistics.median(t_dev),
           max_abs_difference_from_pandas=agree, user_columns=len(proc._unames), item_columns=len(proc._inames))
    del proc, tabs, got, want

    timed(fit_all)
    t_dev = [timed(fit_all)[0] for _ in range(args.repeats)]
    t_pd = []
    for _ in range(args.pandas_repeats):
        t, _ = timed(lambda: (pandas_log_stat(frame), pandas_cond_pop(frame, user_features, "group"),
                              pandas_cond_pop(frame, item_features, "kind")), False)
        t_pd.append(t)
    record("HistoryBasedFeaturesProcessor.fit", t_dev, t_pd, "pandas", rows_per_s_device=n_rows / statistics.median(t_dev))
    del frame

    fp = fit_all()
    n_pairs = args.users * args.candidates
    user = torch.arange(args.users, device=dev).repeat_interleave(args.candidates)
    item = torch.randint(0, args.items, (n_pairs,), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    tabs32 = (fp.log_processor._utab.to(torch.float32), fp.log_processor._itab.to(torch.float32))
    block, names = fp.transform_block(user, item)
    ref = torch_block(fp, user, item, tabs32)
    # the composition works on float32 copies of the tables: its differences round twice, everything else agrees
    close = bool(torch.allclose(block, ref, rtol=1e-5, atol=1e-5))
    del ref, block
    t_dev = [timed(lambda: fp.transform_block(user, item))[0] for _ in range(args.repeats)]
    t_torch = [timed(lambda: torch_block(fp, user, item, tabs32))[0] for _ in range(args.repeats)]
    written = n_pairs * len(names) * 4
    fill = torch.empty((n_pairs, len(names)), dtype=torch.float32, device=dev)
    timed(lambda: fill.fill_(1.0))
    t_fill = statistics.median([timed(lambda: fill.fill_(1.0))[0] for _ in range(args.repeats)])
    more = {"pairs": n_pairs, "columns": len(names), "names": names, "bytes_written": written,
            "written_GBps": written / statistics.median(t_dev) / 1e9, "fill_GBps": written / t_fill / 1e9,
            "fraction_of_fill_rate": t_fill / statistics.median(t_dev), "agrees_with_torch_composition": close}
    if args.hbm_json:
        hbm = json.loads(Path(args.hbm_json).read_text().strip().splitlines()[-1])
        rate = hbm["adam_zero0"]["algorithmic_GBps"]
        more.update(hbm_microbench_adam_GBps=rate, fraction_of_hbm_microbench_rate=more["written_GBps"] / rate)
    record(f"transform_block({args.users} users x {args.candidates}, float32)", t_dev, t_torch, "torch", **more)


if __name__ == "__main__":
    main()
