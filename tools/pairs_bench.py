"""Times the ranking of per-user candidate lists (CQLCore.pairs_topk -> cqlrec_pairs_topk) and, beside it in the same
process, a baseline that is today's composition of predict_pairs(k): the state vectors expanded to one per pair
(`hb.index_select`), `CQLCore.pair_scores` (cqlrec_gather_dot), and a torch top-k per list (`scores.view(users, L)
.topk(k)` -- lists of one length, so the segmented top-k is a plain row-wise one: the cheapest form it can take).

    python tools/pairs_bench.py --shape uniform [--repeats 5] [--out profiles/pairs_bench.json]

    uniform  cfg3's model (100 000 items, d = 128), 1 M users x 100 candidates drawn uniformly
    zipf     the same with Zipf(1)-distributed items
    long     131 072 users x 1 000 candidates, uniform
    d256     1 M items, d = 256, 1 M users x 100 candidates, uniform

k = 10.  Both paths start from the same encoded state vectors (the encoder is common to both and not timed).  If the
baseline's pairs x d block does not fit, the user count is halved for BOTH paths until it does.  Per shape: one warm-up
of each path, then alternating repeats (device events around the whole call, the host waits on the last event); median
and spread (max - min) of each, pairs/s, and gathered E_out bytes/s = pairs * 2 d / time beside the chip's measured
row-gather rates (MI355X: 8.6 TB/s for a 38 MB table served from the Infinity Cache, 5.5-5.8 TB/s from HBM; both
measured on rows of 1 152 B and more, these rows are 256 and 512 B).  Needs a GPU; one process per shape."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

# name: (items, d, users, candidates per user, zipf)
SHAPES = {"uniform": (100_000, 128, 1_000_000, 100, False), "zipf": (100_000, 128, 1_000_000, 100, True),
          "long": (100_000, 128, 131_072, 1_000, False), "d256": (1_000_000, 256, 1_000_000, 100, False),
          "tiny": (5_000, 64, 4_096, 50, False)}
GATHER_CACHE, GATHER_HBM = 8.6e12, 5.5e12      # guide figures: table inside / beyond the 256 MiB Infinity Cache


def candidate_lists(users, per, n_items, zipf, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((users, per), dtype=torch.int32, device="cuda")
    step = max(1, (1 << 26) // per)
    mult = 2654435761 % n_items
    while math.gcd(mult, n_items) != 1:
        mult += 1
    for lo in range(0, users, step):
        hi = min(users, lo + step)
        if zipf:      # rank ~ Zipf(1) through a fixed affine permutation of the ids (data.synth_log_device's generator)
            u = torch.rand((hi - lo, per), generator=g, device="cuda", dtype=torch.float64)
            r = torch.floor(torch.exp(u * math.log(n_items + 1.0))).to(torch.int64).clamp_(1, n_items) - 1
            it = (r * mult + 12345) % n_items
        else:
            it = torch.randint(0, n_items, (hi - lo, per), generator=g, device="cuda")
        out[lo:hi] = torch.sort(it, dim=1)[0].to(torch.int32)
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="JSON file to merge this shape's result into")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pairs_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd.core import CQLCore, CQLHyper
    n_items, d, users, per, zipf = SHAPES[args.shape]
    k = args.k
    core = CQLCore(n_items, CQLHyper(d=d), device="cuda:0")
    g = torch.Generator(device="cuda").manual_seed(7)
    E = core.segment(core.theta, "E_out")
    for lo in range(0, n_items, 65536):
        E[lo: lo + 65536] = 0.1 * torch.randn(E[lo: lo + 65536].shape, generator=g, device="cuda")
    core.refresh_shadows()

    while True:
        try:
            items = candidate_lists(users, per, n_items, zipf)
            hb = torch.randn((users, d), generator=g, device="cuda").to(torch.bfloat16)
            off = torch.arange(users + 1, dtype=torch.int64, device="cuda") * per
            flat = items.view(-1)
            inv = torch.arange(users, device="cuda").repeat_interleave(per)

            def old():
                s = core.pair_scores(hb.index_select(0, inv), flat)
                v, j = s.view(users, per).topk(k, dim=1)
                return items.gather(1, j).int(), v
            t_warm_old, (bi, bv) = timed(old)
            break
        except torch.cuda.OutOfMemoryError:
            items = hb = off = flat = inv = None
            torch.cuda.empty_cache()
            users //= 2
            if users < 1024:
                raise

    new = lambda: core.pairs_topk(hb, off, flat, None, k)         # noqa: E731
    _, (ni, nv, nc) = timed(new)
    same_val = float((nv == bv).float().mean())                   # torch.topk breaks ties in its own way: compare values
    same_idx = float((ni == bi).float().mean())
    t_new, t_old = [], []
    for _ in range(args.repeats):                                 # alternating
        t_new.append(timed(new)[0])
        t_old.append(timed(old)[0])
    nnz = users * per
    m_new, m_old = statistics.median(t_new), statistics.median(t_old)
    s_new, s_old = max(t_new) - min(t_new), max(t_old) - min(t_old)
    table_bytes = n_items * d * 2
    guide = GATHER_CACHE if table_bytes <= (256 << 20) else GATHER_HBM
    row = {"shape": args.shape, "n_items": n_items, "d": d, "users": users, "candidates_per_user": per, "zipf": zipf, "k": k,
           "pairs": nnz, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "new_s": t_new, "baseline_s": t_old, "new_median_s": m_new, "baseline_median_s": m_old,
           "new_spread_s": s_new, "baseline_spread_s": s_old, "pairs_per_s": nnz / m_new,
           "baseline_pairs_per_s": nnz / m_old, "gathered_bytes_per_s": nnz * 2 * d / m_new,
           "baseline_gathered_bytes_per_s": nnz * 2 * d / m_old, "table_bytes": table_bytes,
           "guide_gather_bytes_per_s": guide, "fraction_of_guide_gather_rate": nnz * 2 * d / m_new / guide,
           "speedup": m_old / m_new, "not_slower_than_baseline": bool(m_new <= m_old),
           "faster_by_more_than_the_spreads": bool(min(t_old) - max(t_new) > 0 and m_old - m_new > s_new + s_old),
           "values_equal_to_baseline": same_val, "ids_equal_to_baseline": same_idx,
           "baseline_intermediate_bytes": nnz * d * 2}
    print(json.dumps({k_: v for k_, v in row.items() if k_ not in ("new_s", "baseline_s")}), flush=True)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        blob = json.loads(path.read_text()) if path.exists() else {}
        blob[args.shape] = row
        path.write_text(json.dumps(blob, indent=1) + "\n")


if __name__ == "__main__":
    main()
