"""Times ALS (replay_cql_amd.als -> csrc/als.hip) on the cfg3 log and puts two floors the tool computes itself beside
every time.

    python tools/als_bench.py [--users 1000000] [--items 100000] [--ranks 10 128] [--repeats 5] [--k 10]
                              [--out profiles/als_bench.json]

The log is tools/bench_record.make_log's (1 M users, 100 000 items, about 48 M rows, device columns in, fixed random row
order).  Timed per rank, each as the median of `repeats` whole calls after one warm-up (host clock around a call that
ends in a device synchronise), with the spread (max - min):
  one iteration            Gram matrix + item half step + Gram matrix + user half step, on the two CSR views built once
  its four parts           the same calls one by one
  ALSWrap.fit(max_iter=1)  the whole call: id checks, both segment sorts, the initial draw and one iteration
  recommend, k = 10        every user of the log, seen items filtered; device columns in and out

Nobody has measured ALS on this device before, so there is no target.  The floors of ONE iteration:
  gather   2 nnz rank 4 bytes -- every entry gathers one fp32 factor row, once per side -- over the slowest and the
           fastest gather rate recorded in profiles/pairs_bench.json (its non-tiny shapes)
  fp64     2 nnz r (r + 1) + (n_users + n_items) r^3 / 3 operations over the fp64 vector peak: 78.6 TFLOP/s, half of the
           fp32 vector peak the microarchitecture guide states (157.3 TFLOP/s spec), as CDNA4 issues fp64 FMAs
The floor of recommend is the dense score: n_users n_items rank fp32 FMAs over the fp32 vector peak.  Needs a GPU."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.bench_record import Recorder, make_log, repeat          # noqa: E402  pylint: disable=wrong-import-position

FP32_VECTOR_PEAK = 157.3e12
FP64_VECTOR_PEAK = FP32_VECTOR_PEAK / 2


def gather_rates():
    rows = json.loads((ROOT / "profiles" / "pairs_bench.json").read_text())
    rates = [v["gathered_bytes_per_s"] for k, v in rows.items() if isinstance(v, dict) and k != "tiny" and
             "gathered_bytes_per_s" in v]
    return min(rates), max(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--ranks", type=int, nargs="+", default=[10, 128])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("als_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd import _log as L
    from replay_cql_amd import als as A
    dev = torch.device("cuda:0")
    log = make_log(args.users, args.items, dev)
    nnz = int(log["user_idx"].numel())
    slow, fast = gather_rates()
    result = {"device": torch.cuda.get_device_name(0), "users": args.users, "items": args.items, "rows": nnz,
              "repeats": args.repeats, "k": args.k, "piece": A.PIECE, "gather_rates_bytes_per_s": [slow, fast],
              "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "fp32_vector_peak_flops": FP32_VECTOR_PEAK, "ranks": {}}

    rec = Recorder(result, args.out, calls={})
    record = rec.record

    def times_of(fn):
        return repeat(fn, args.repeats)[0]

    # the two CSR views, as ALSWrap._fit_device builds them
    eng = A.Als(dev)
    lg = L.open_log(log, "als_bench")
    (user, n_users), (item, n_items) = L.dense_ids(lg, ["user_idx", "item_idx"])
    rel = L.float_column(lg, "relevance")
    item_side, user_side = eng.view(item, n_items, user, rel)[0], eng.view(user, n_users, item, rel)[0]
    off_i, off_u = item_side[0], user_side[0]
    np_i, np_u = A.count_pieces(off_i), A.count_pieces(off_u)
    result.update(item_pieces=np_i, user_pieces=np_u, longest_item_row=int((off_i[1:] - off_i[:-1]).max().item()),
                  longest_user_row=int((off_u[1:] - off_u[:-1]).max().item()))

    for r in args.ranks:
        model = A.ALSWrap(rank=r, seed=1, max_iter=1)
        U = model._init_factors(n_users, r, 1, dev)
        V = torch.zeros((n_items, r), dtype=torch.float32, device=dev)
        has_u, has_v = torch.ones(n_users, dtype=torch.uint8, device=dev), torch.zeros(n_items, dtype=torch.uint8, device=dev)
        failed = torch.zeros(1, dtype=torch.int32, device=dev)

        def item_step():
            eng.half_step(item_side, U, eng.gram(U), True, 1.0, 0.1, V, has_v, failed, n_pieces=np_i)

        def user_step():
            eng.half_step(user_side, V, eng.gram(V), True, 1.0, 0.1, U, has_u, failed, n_pieces=np_u)

        def iteration():
            item_step()
            user_step()

        gather_bytes = 2 * nnz * r * 4
        fp64_ops = 2 * nnz * r * (r + 1) + (n_users + n_items) * r ** 3 / 3
        floors = {"gather_bytes": gather_bytes, "gather_floor_s": [gather_bytes / fast, gather_bytes / slow],
                  "fp64_ops": fp64_ops, "fp64_floor_s": fp64_ops / FP64_VECTOR_PEAK}
        row = {"floors_of_one_iteration": floors, "calls": {}}
        result["ranks"][str(r)] = row
        rec.calls, rec.tag = row["calls"], {"rank": r}

        times = times_of(iteration)
        med = statistics.median(times)
        floor = max(floors["gather_floor_s"][0], floors["fp64_floor_s"])
        record("iteration", times, over_gather_floor=[med / f for f in floors["gather_floor_s"]],
               over_fp64_floor=med / floors["fp64_floor_s"], over_larger_floor=med / floor, failed=int(failed.item()))
        record("gram(user factors)", times_of(lambda: eng.gram(U)))
        record("gram(item factors)", times_of(lambda: eng.gram(V)))
        G_u, G_v = eng.gram(U), eng.gram(V)
        record("half_step(items)", times_of(lambda: eng.half_step(item_side, U, G_u, True, 1.0, 0.1, V, has_v, failed, n_pieces=np_i)),
               fp64_floor_s=(nnz * r * (r + 1) + n_items * r ** 3 / 3) / FP64_VECTOR_PEAK)
        record("half_step(users)", times_of(lambda: eng.half_step(user_side, V, G_v, True, 1.0, 0.1, U, has_u, failed, n_pieces=np_u)),
               fp64_floor_s=(nnz * r * (r + 1) + n_users * r ** 3 / 3) / FP64_VECTOR_PEAK)

        def fit():
            mm = A.ALSWrap(rank=r, seed=1, max_iter=1)
            mm.fit(log)
            return mm

        times, model = repeat(fit, args.repeats)
        record("ALSWrap.fit(max_iter=1)", times)

        score_floor = args.users * args.items * r / (FP32_VECTOR_PEAK / 2)          # FMAs per second = FLOP/s / 2
        times = times_of(lambda: model.recommend(log, args.k))
        med = statistics.median(times)
        record(f"recommend(all users, k={args.k})", times, score_fmas=args.users * args.items * r, fp32_floor_s=score_floor,
               over_fp32_floor=med / score_floor, users_per_s=args.users / med)
        del model, U, V


if __name__ == "__main__":
    main()
