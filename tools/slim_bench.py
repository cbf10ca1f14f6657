"""Times SLIM (replay_cql_amd.slim -> section f12, csrc/slim.hip) on cuts of the cfg3 log.

    python tools/slim_bench.py [--fit-items 16384 4096] [--repeats 5] [--out profiles/slim_bench.json]

The cfg3 log (tools/bench_record.make_log: 1 M users, 100 000 items, about 48 M rows) is cut with the package's own
filter_by_min_count and Indexer to the largest catalogue of at most n items (a tie at the cut would add items, so the
threshold moves up by one count where it must): n = CQLREC_SLIM_MAX_ITEMS, where G is 2 GiB and every update streams a
128 KB row from HBM, and n = 4096, where G (128 MiB) sits in the 256 MiB Infinity Cache.

Per cut, at the reference's defaults (beta = lambda_ = 0.01, tol 1e-4), each time the median of `repeats` whole calls
after one warm-up (host clock around a call that ends in a device synchronise), with the spread (max - min):
  SLIM().fit                 the whole fit, with sweeps per column (median / max), the total of non-zero updates, the
                             bytes of G rows those updates and the refreshes read, and that count over the solver's time
                             beside the chip's measured streaming rate (profiles/README.md: 4.87 TB/s, Adam over 268 M
                             parameters) -- the floor of this design is its row traffic at that rate
  dense_gram / slim_fit / admm_compact      the three pieces alone, and their shares of the fit
If scikit-learn imports, the reference's ElasticNet (replay/models/slim.py's settings) is timed on 32 evenly spaced
columns of the same matrix on the host and extrapolated to the whole catalogue.  Needs a GPU."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.bench_record import Recorder, make_log, repeat as bench_repeat          # noqa: E402  pylint: disable=wrong-import-position

STREAMING_TBPS = 4.87          # profiles/README.md, r02_hbm_traffic.json: Adam over 268 M parameters, 0.61 of the nominal 8 TB/s


def sklearn_columns(small, n_users, n_items, beta, lambda_, columns, budget_s):
    """seconds per column of the reference's ElasticNet on the host (as many of `columns` as fit `budget_s`), or None
    without scikit-learn"""
    try:
        import numpy as np
        from scipy.sparse import csc_matrix
        from sklearn.linear_model import ElasticNet
    except ImportError:
        return None
    import warnings
    X = csc_matrix((small["relevance"].cpu().numpy(), (small["user_idx"].cpu().numpy().astype(np.int64),
                                                       small["item_idx"].cpu().numpy().astype(np.int64))), shape=(n_users, n_items))
    alpha = beta + lambda_
    model = ElasticNet(alpha=alpha, l1_ratio=lambda_ / alpha, fit_intercept=False, max_iter=5000, random_state=0,
                       selection="random", positive=True)
    times, begun = [], time.perf_counter()
    for j in columns:
        lo, hi = X.indptr[j], X.indptr[j + 1]
        y = np.zeros(n_users)
        y[X.indices[lo:hi]] = X.data[lo:hi]
        kept = X.data[lo:hi].copy()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            X.data[lo:hi] = 0.0                               # the reference zeroes column j of the matrix for the fit
            model.fit(X, y)
            X.data[lo:hi] = kept
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - begun > budget_s:
            break
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--fit-items", type=int, nargs="*", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-columns", type=int, default=32)
    ap.add_argument("--sklearn-budget-s", type=float, default=90.0, help="no further column is begun after this many seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slim_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd import _native as N
    from replay_cql_amd._dense import Dense
    from replay_cql_amd import slim as SL
    from replay_cql_amd.filters import filter_by_min_count
    from replay_cql_amd.indexer import Indexer
    dev = torch.device("cuda:0")
    D = Dense(dev)
    sizes = args.fit_items or [N.SLIM_MAX_ITEMS, 4096]
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "streaming_tbps": STREAMING_TBPS,
              "defaults": {"beta": 0.01, "lambda_": 0.01, "tol": SL.SLIM.tol, "max_iter": SL.SLIM.max_iter}, "calls": {}}

    rec = Recorder(result, args.out)
    record, save = rec.record, rec.save

    def repeat(fn):
        return bench_repeat(fn, args.repeats)

    log = make_log(args.users, args.items, dev)
    counts = torch.bincount(log["item_idx"].long(), minlength=args.items)
    ranked = torch.sort(counts, descending=True).values
    for n in sizes:
        threshold = int(ranked[n - 1].item())
        if int((counts >= threshold).sum().item()) > n:          # a tie at the cut: the catalogue must not exceed n
            threshold += 1
        cut = filter_by_min_count(log, threshold, "item_idx")
        raw = {"user_id": cut["user_idx"], "item_id": cut["item_idx"], "relevance": cut["relevance"]}
        indexer = Indexer()
        indexer.fit(raw, raw)
        small = indexer.transform(raw)
        n_items = int(small["item_idx"].max().item()) + 1
        n_users = int(small["user_idx"].max().item()) + 1
        g_bytes = 8 * n_items * n_items
        shape = {"items": n_items, "users": n_users, "rows": int(small["item_idx"].numel()), "min_count": threshold,
                 "G_bytes": g_bytes, "regime": "Infinity Cache resident" if g_bytes <= 256 << 20 else "HBM streaming"}

        def fit():
            m = SL.SLIM()
            m.fit(small)
            return m
        times, model = repeat(fit)
        sweeps = model.n_sweeps.cpu().numpy()
        fit_s = record(f"SLIM().fit items={n}", times, sweeps_median=float(statistics.median(sweeps.tolist())),
                       sweeps_max=int(sweeps.max()), updates=model.n_updates, not_converged=model.n_not_converged,
                       kkt_max=float(model.kkt.max().item()), table_nnz=int(model.similarity_device[1].numel()), **shape)

        item, user = small["item_idx"], small["user_idx"]
        rel = small["relevance"].to(torch.float64)
        views = (D.view(item, n_items, user, rel)[0], D.view(user, n_users, item, rel)[0])
        times, G = repeat(lambda: D.gram(*views, n_items, n_users))
        gram_s = record(f"dense_gram items={n}", times)
        del views
        S = torch.zeros((n_items, n_items), dtype=torch.float64, device=dev)
        solver = SL.SLIM()
        times, out = repeat(lambda: solver.solve(D, G, n_users, S=S))
        # rows of G read: one per update, and per sweep of a column the row of the column plus one per support entry; the
        # support at each refresh is not kept, the final one stands in for it (it grows towards it)
        support = (out[0] != 0).sum(dim=0).to(torch.int64)
        refresh_rows = int((out[1].to(torch.int64) * (1 + support)).sum().item())
        row_bytes = 8 * n_items * (int(out[3].sum().item()) + refresh_rows + n_items)
        solve_s = record(f"slim_fit items={n}", times, updates=int(out[3].sum().item()), refresh_rows=refresh_rows,
                         G_row_bytes_read=row_bytes, row_TBps=row_bytes / statistics.median(times) / 1e12,
                         of_streaming_rate=row_bytes / statistics.median(times) / 1e12 / STREAMING_TBPS,
                         floor_s_at_streaming_rate=row_bytes / (STREAMING_TBPS * 1e12))
        times, _ = repeat(lambda: D.to_csr(S))
        csr_s = record(f"admm_compact items={n}", times)
        result.setdefault("shares", {})[f"items={n}"] = {"gram": gram_s / fit_s, "slim_fit": solve_s / fit_s, "csr": csr_s / fit_s,
                                                          "rest (ids, segments, the three result vectors)": 1 - (gram_s + solve_s + csr_s) / fit_s}
        del G, S, out
        columns = [int(round(x)) for x in torch.linspace(0, n_items - 1, args.sklearn_columns).tolist()] if args.sklearn_columns else []
        columns = columns[::2] + columns[1::2]              # a budget that runs out still leaves evenly spaced columns
        per_column = sklearn_columns(small, n_users, n_items, 0.01, 0.01, columns, args.sklearn_budget_s) if columns else None
        if per_column:
            mean = sum(per_column) / len(per_column)
            result["calls"][f"sklearn ElasticNet items={n}"] = {
                "columns": len(per_column), "s_per_column_mean": mean, "s_per_column_max": max(per_column),
                "extrapolated_fit_s": mean * n_items, "over_SLIM_fit": mean * n_items / fit_s}
            print(json.dumps({"call": f"sklearn ElasticNet items={n}", **result["calls"][f"sklearn ElasticNet items={n}"]}), flush=True)
        del model, small, cut, raw
        save()
    print(json.dumps({"shares": result.get("shares", {})}), flush=True)
    save()


if __name__ == "__main__":
    main()
