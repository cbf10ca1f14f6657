"""Times the association rules (replay_cql_amd.association_rules -> section f10 of csrc/neighbour.hip) on the cfg3 log
and, beside them in the same process, their two yardsticks: ItemKNN(10).fit on the same log (the same expansion, one
value plane instead of three, no dedup in front) and the radix sort of as many tuples alone.

    python tools/rules_bench.py [--users 1000000] [--items 100000] [--repeats 5] [--out profiles/rules_bench.json]

The log is tools/bench_record.make_log's, as in tools/neighbour_bench.py (1 M users, 100 000 items, about 48 M rows, device
columns in, fixed random row order); sessions are the users.  Timed, each as the median of `repeats` whole calls after
one warm-up (host clock around a call that ends in a device synchronise), with the spread (max - min):
  AssociationRulesItemRec().fit                                   the defaults: min_item_count = min_pair_count = 5, k = 1000
  AssociationRulesItemRec().recommend, k = 10                     every user of the log, seen items filtered, by confidence
  AssociationRulesItemRec(min_item_count=1, min_pair_count=1).fit every item and every pair
  ItemKNN(10).fit                                                 weighting None
  sort_alone                                                      torch.sort over chunks of max_tuples random int64 keys, as
                                                                  many tuples as the unfiltered rules fit expands to
With each fit: the tuples expanded, the chunks they were cut into, the pairs kept; at the end the three ratios: each
rules fit over ItemKNN's, and the unfiltered rules fit over the sort floor.  Needs a GPU."""
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

from tools.bench_record import Recorder, make_log, repeat as bench_repeat          # noqa: E402  pylint: disable=wrong-import-position


def chunk_count(prefix, max_tuples: int) -> int:
    """the chunks cqlrec_rules_topk cuts the rows of a host row prefix into: consecutive rows while their tuples fit"""
    prefix = prefix.tolist()
    n_q, q0, chunks = len(prefix) - 1, 0, 0
    while q0 < n_q:
        q1 = q0 + 1
        while q1 < n_q and prefix[q1 + 1] - prefix[q0] <= max_tuples:
            q1 += 1
        chunks += prefix[q1] > prefix[q0]
        q0 = q1
    return chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--max-tuples", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rules_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd import neighbour as NB
    from replay_cql_amd.association_rules import AssociationRulesItemRec
    dev = torch.device("cuda:0")
    log = make_log(args.users, args.items, dev)
    n_rows = int(log["user_idx"].numel())
    max_tuples = args.max_tuples or NB.DEFAULT_MAX_TUPLES
    result = {"device": torch.cuda.get_device_name(0), "users": args.users, "items": args.items, "rows": n_rows,
              "repeats": args.repeats, "k": args.k, "max_tuples": max_tuples, "calls": {}}

    rec = Recorder(result, args.out)
    record, save = rec.record, rec.save

    def repeat(fn):
        return bench_repeat(fn, args.repeats)

    def rules(**more):
        model = AssociationRulesItemRec(max_tuples=max_tuples, **more)
        model.fit(log)
        return model

    def fit_case(name, **more):
        times, model = repeat(lambda: rules(**more))
        total, largest = model.expansion
        record(name, times, distinct_rows=int(model.item_count.sum().item()), num_sessions=model.num_sessions,
               expansion_tuples=total, largest_row_tuples=largest,
               chunks=chunk_count(model.row_prefix, min(max_tuples, max(1, total))),
               kept_pairs=int(model.similarity_device[4].sum().item()), num_neighbours=model.similarity_device[0].shape[1],
               tuples_per_s=total / statistics.median(times), rows_per_s=n_rows / statistics.median(times))
        return model

    model = fit_case("AssociationRulesItemRec().fit")
    times, out = repeat(lambda: model.recommend(log, args.k))
    total, largest = model.expansion
    record(f"AssociationRulesItemRec().recommend(all users, k={args.k})", times, metric=model.similarity_metric,
           expansion_tuples=total, largest_row_tuples=largest, rows_out=int(out["item_idx"].numel()),
           users_per_s=args.users / statistics.median(times))
    del model, out
    model = fit_case("AssociationRulesItemRec(min_item_count=1, min_pair_count=1).fit", min_item_count=1, min_pair_count=1)
    rules_tuples = model.expansion[0]
    del model

    def knn():
        m = NB.ItemKNN(10, max_tuples=max_tuples)
        m.fit(log)
        return m
    times, m = repeat(knn)
    total, largest = m.expansion
    record("ItemKNN(10).fit", times, expansion_tuples=total, largest_row_tuples=largest,
           tuples_per_s=total / statistics.median(times), chunks_at_least=-(-total // max_tuples))
    del m

    # the sort alone: as many tuples as the unfiltered rules fit expands to, in chunks of max_tuples
    gen = torch.Generator(device=dev).manual_seed(3)
    chunk = max(1, min(max_tuples, rules_tuples))
    keys = torch.randint(0, 1 << 62, (chunk,), device=dev, generator=gen)
    n_chunks = -(-rules_tuples // chunk)
    per_chunk, _ = repeat(lambda: torch.sort(keys))
    del keys
    record("sort_alone(torch.sort, int64 keys + int64 index, 64 bits)", [t * n_chunks for t in per_chunk],
           tuples=rules_tuples, chunk_tuples=chunk, chunks=n_chunks, per_chunk_median_s=statistics.median(per_chunk))

    med = {k: v["median_s"] for k, v in result["calls"].items()}
    result["ratios"] = {
        "rules_fit_defaults_over_item_knn_fit": med["AssociationRulesItemRec().fit"] / med["ItemKNN(10).fit"],
        "rules_fit_unfiltered_over_item_knn_fit":
            med["AssociationRulesItemRec(min_item_count=1, min_pair_count=1).fit"] / med["ItemKNN(10).fit"],
        "rules_fit_unfiltered_over_sort_alone":
            med["AssociationRulesItemRec(min_item_count=1, min_pair_count=1).fit"] /
            med["sort_alone(torch.sort, int64 keys + int64 index, 64 bits)"],
    }
    print(json.dumps({"ratios": result["ratios"]}), flush=True)
    save()


if __name__ == "__main__":
    main()
