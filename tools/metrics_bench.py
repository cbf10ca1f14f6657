"""Times the evaluation of a recommendation frame on the device (replay_cql_amd.metrics, csrc/metrics.hip): frame -> block
and the eleven metrics at U users x k rows each, ks = {1, 5, 10}, and, beside it, the CPU restatement of tests/ at a size
that finishes (a Python loop per user: its rate is a floor for "what the host does", not a tuned baseline).

    python tools/metrics_bench.py [--users 1000000] [--k 10] [--repeats 5] [--cpu-users 2000] [--out profiles/metrics_bench.json]

Each GPU figure: one warm-up, then `repeats` calls with a device synchronise before the clock stops (the classes read
their sums back, which synchronises as well); median and spread (max - min).  The times are end-to-end calls (column
set-up, user-set search, workspace allocation, kernels, read-back), not kernel times.  No threshold is set anywhere:
this records what the device gives.  Needs a GPU; there is no CPU path for the device figures."""
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

KS = [1, 5, 10]


def frames(n_users, k, n_items, seed=0):
    """numpy columns of a shuffled frame with k rows per user (Zipf items, so users repeat popular ones; relevance with
    ties), a ground truth of 0..3 rows per user, a base prediction frame and previous-policy weights"""
    rng = np.random.default_rng(seed)
    user = np.repeat(np.arange(n_users, dtype=np.int32), k)
    item = np.clip(rng.zipf(1.2, len(user)) - 1, 0, n_items - 1).astype(np.int32)
    rel = np.round(rng.normal(size=len(user)), 2)
    p = rng.permutation(len(user))
    recs = {"user_idx": user[p], "item_idx": item[p], "relevance": rel[p]}
    gu = np.repeat(np.arange(n_users, dtype=np.int32), rng.integers(0, 4, n_users))
    gt = {"user_idx": gu, "item_idx": np.clip(rng.zipf(1.2, len(gu)) - 1, 0, n_items - 1).astype(np.int32)}
    base = {"user_idx": user, "item_idx": rng.integers(0, n_items, len(user)).astype(np.int32),
            "relevance": rng.normal(size=len(user))}
    prev = {"user_idx": user[p][::2].copy(), "item_idx": item[p][::2].copy(), "relevance": rng.random(len(user[::2])) + 0.1}
    return recs, gt, base, prev


def to_device(cols):
    return {k: torch.as_tensor(v).cuda() for k, v in cols.items()}


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-users", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd import metrics as M
    from tests import metrics_reference as R
    ks = [k for k in KS if k <= args.k]
    recs_h, gt_h, base_h, prev_h = frames(args.users, args.k, args.items)
    recs, gt, base, prev = (to_device(c) for c in (recs_h, gt_h, base_h, prev_h))
    users = {"user_idx": torch.arange(args.users, dtype=torch.int32, device="cuda")}
    ut = torch.arange(args.users, dtype=torch.int64, device="cuda")
    rows = M._rows_of(ut, recs["user_idx"])                               # pylint: disable=protected-access
    metrics = {n: getattr(M, n)() for n in M.METRICS + ("RocAuc",)}
    metrics["NCISPrecision"] = M.NCISPrecision(prev, activation="softmax")
    calls = {"frame_to_block": lambda: M.frame_to_block(rows, recs["item_idx"], recs["relevance"], args.users, args.k,
                                                        want_pos=True)}
    for name, metric in metrics.items():
        calls[name] = lambda m=metric: m(recs, gt, ks, users)
    sur, unexp, cov = M.Surprisal(gt), M.Unexpectedness(base), M.Coverage(gt)
    calls["Surprisal"] = lambda: sur(recs, ks, users)
    calls["Unexpectedness"] = lambda: unexp(recs, ks, users)
    calls["Coverage"] = lambda: cov(recs, ks, users)
    calls["item_distribution"] = lambda: M.item_distribution(gt, recs, args.k)
    result = {"users": args.users, "k": args.k, "ks": ks, "items": args.items, "rows": int(recs["item_idx"].numel()),
              "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "gpu": {}}
    for name, fn in calls.items():
        t = timed(fn, args.repeats)
        row = {"s": t, "median_s": statistics.median(t), "spread_s": max(t) - min(t),
               "users_per_s": args.users / statistics.median(t)}
        result["gpu"][name] = row
        print(json.dumps({"call": name, **{k: v for k, v in row.items() if k != "s"}}), flush=True)
    # the CPU restatement on the first --cpu-users users of the same frames
    n = args.cpu_users
    sel = lambda c, cols: [list(r) for r in zip(*(c[x][c["user_idx"] < n].tolist() for x in cols))]       # noqa: E731
    fr = sel(recs_h, ("user_idx", "item_idx", "relevance"))
    g = [r + [1.0] for r in sel(gt_h, ("user_idx", "item_idx"))]
    t = time.perf_counter()
    R.frame_to_block(fr, list(range(n)), args.k)
    t_block = time.perf_counter() - t
    cpu = {"users": n, "frame_to_block_s": t_block, "frame_to_block_users_per_s": n / t_block}
    for name in ("NDCG", "RocAuc", "Surprisal"):
        t = time.perf_counter()
        R.per_user_values(name, fr, ks, gt=g, gt_users=list(range(n)), log=g)
        cpu[name + "_s"] = time.perf_counter() - t
        cpu[name + "_users_per_s"] = n / cpu[name + "_s"]
    result["cpu_restatement"] = cpu
    print(json.dumps({"cpu_restatement": cpu}), flush=True)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
