"""Times the neighbourhood model (replay_cql_amd.neighbour -> csrc/neighbour.hip) on the cfg3 log and, beside it in the
same process, the two yardsticks of its design: the radix sort of as many tuples alone, and a torch.sparse composition.

    python tools/neighbour_bench.py [--users 1000000] [--items 100000] [--repeats 5] [--baseline-blocks 4]
                                    [--block-rows 1000] [--out profiles/neighbour_bench.json]

The log is tools/bench_record.make_log's (1 M users, 100 000 items, about 48 M rows, device columns in, fixed random row
order).  Timed, each as the median of `repeats` whole calls after one warm-up (host clock around a call that ends in a
device synchronise), with the spread (max - min):
  ItemKNN(10).fit                 weighting None and bm25; device columns in, the similarity block on the device out
  ItemKNN.recommend, k = 10       every user of the log, seen items filtered; device columns in and out
With each: the expansion (the tuples of the sparse product) and tuples per second.

The floor of the design -- expand, SORT, reduce, select -- is the sort: `sort_alone` is torch.sort (rocPRIM's radix sort
of (int64 key, int64 index) pairs, all 64 bits) over chunks of max_tuples random keys, as many tuples as the fit expands
to.  It moves the same bytes per tuple as the engine's first sort but passes over all 64 bits, where the engine sorts
only the bits its keys use; the engine then sorts each chunk twice more to select.

The baseline returns the same rows by torch.sparse.mm + topk: for a block of `block-rows` items, (block x users) @ (users
x items) as sparse x sparse, made dense (block x items), divided by the norms, the diagonal masked, topk(10).  Only
`baseline-blocks` blocks are run; the whole fit is their median times the number of blocks (stated as extrapolated).
Duplicated (user, item) rows are summed by the coalesce there, which the model keeps apart: a yardstick of cost, not of
values.  Needs a GPU."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.bench_record import Recorder, make_log, timed, repeat as bench_repeat          # noqa: E402  pylint: disable=wrong-import-position


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--max-tuples", type=int, default=None)
    ap.add_argument("--baseline-blocks", type=int, default=4)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbour_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd import neighbour as NB
    dev = torch.device("cuda:0")
    log = make_log(args.users, args.items, dev)
    n_rows = int(log["user_idx"].numel())
    max_tuples = args.max_tuples or NB.DEFAULT_MAX_TUPLES
    result = {"device": torch.cuda.get_device_name(0), "users": args.users, "items": args.items, "rows": n_rows,
              "repeats": args.repeats, "neighbours": args.neighbours, "k": args.k, "max_tuples": max_tuples, "calls": {}}

    record = Recorder(result, args.out).record

    def repeat(fn):
        return bench_repeat(fn, args.repeats)

    def fit(weighting):
        model = NB.ItemKNN(args.neighbours, weighting=weighting, max_tuples=max_tuples)
        model.fit(log)
        return model

    model = None
    for weighting in (None, "bm25"):
        times, model = repeat(lambda: fit(weighting))
        total, largest = model.expansion
        record(f"ItemKNN.fit(weighting={weighting})", times, expansion_tuples=total, largest_row_tuples=largest,
               tuples_per_s=total / statistics.median(times), rows_per_s=n_rows / statistics.median(times),
               chunks_at_least=-(-total // max_tuples))
    fit_tuples = model.expansion[0]

    times, out = repeat(lambda: model.recommend(log, args.k))
    total, largest = model.expansion
    record(f"ItemKNN.recommend(all users, k={args.k})", times, expansion_tuples=total, largest_row_tuples=largest,
           tuples_per_s=total / statistics.median(times), rows_out=int(out["item_idx"].numel()),
           users_per_s=args.users / statistics.median(times))
    del out

    # the sort alone: as many tuples as the fit expands to, in chunks of max_tuples
    gen = torch.Generator(device=dev).manual_seed(3)
    chunk = min(max_tuples, fit_tuples)
    keys = torch.randint(0, 1 << 62, (chunk,), device=dev, generator=gen)
    n_chunks = -(-fit_tuples // chunk)
    per_chunk = repeat(lambda: torch.sort(keys))[0]
    del keys
    record("sort_alone(torch.sort, int64 keys + int64 index, 64 bits)", [t * n_chunks for t in per_chunk],
           tuples=fit_tuples, chunk_tuples=chunk, chunks=n_chunks, per_chunk_median_s=statistics.median(per_chunk),
           tuples_per_s=chunk / statistics.median(per_chunk))

    # the torch.sparse composition, a few blocks of item rows
    user, item = log["user_idx"].long(), log["item_idx"].long()
    ones = torch.ones(n_rows, dtype=torch.float64, device=dev)
    A = torch.sparse_coo_tensor(torch.stack([user, item]), ones, (args.users, args.items)).coalesce()
    norm = torch.sqrt(torch.zeros(args.items, dtype=torch.float64, device=dev).index_add_(0, item, ones))
    order = torch.argsort(item)
    item_s, user_s = item[order], user[order]
    bounds = torch.searchsorted(item_s, torch.arange(0, args.items + args.block_rows, args.block_rows, device=dev)).tolist()
    n_blocks = -(-args.items // args.block_rows)

    def block(b):
        lo, hi = bounds[b], bounds[b + 1]
        rows = min(args.block_rows, args.items - b * args.block_rows)
        At = torch.sparse_coo_tensor(torch.stack([item_s[lo:hi] - b * args.block_rows, user_s[lo:hi]]), ones[lo:hi],
                                     (rows, args.users)).coalesce()
        C = torch.sparse.mm(At, A).to_dense()
        reached = C != 0
        C = C / (norm[b * args.block_rows:b * args.block_rows + rows, None] * norm[None, :])
        C = torch.where(reached, C, torch.full_like(C, -float("inf")))
        C[torch.arange(rows, device=dev), torch.arange(rows, device=dev) + b * args.block_rows] = -float("inf")
        return torch.topk(C, args.neighbours, dim=1)

    try:
        picks = [int(b) for b in torch.linspace(0, n_blocks - 1, args.baseline_blocks).tolist()]
        timed(lambda: block(picks[0]))
        per_block = [timed(lambda: block(b))[0] for b in picks]
        record(f"torch.sparse.mm + topk, blocks of {args.block_rows} item rows", per_block, blocks_timed=picks,
               blocks_in_all=n_blocks, extrapolated_fit_s=statistics.median(per_block) * n_blocks,
               over_device_fit=statistics.median(per_block) * n_blocks /
               result["calls"]["ItemKNN.fit(weighting=None)"]["median_s"])
    except RuntimeError as err:                            # a torch build without sparse x sparse on this device
        record("torch.sparse.mm + topk", [float("nan")], error=str(err)[:300])


if __name__ == "__main__":
    main()
