"""Times item-to-item nearest neighbours (CQLCore.item_knn -> cqlrec_item_knn) at the two timed catalogue shapes and,
beside it, a baseline that is NOT the code under test: the same answer from torch.matmul on bf16 query chunks, the
metric's epilogue in torch and torch.topk (the Q x C chunk is materialised in fp32).

    python tools/knn_bench.py --shape cfg3 [--metric cosine_similarity ...] [--repeats 5] [--out profiles/knn_bench.json]

    cfg3  N = 100 000, d = 128, every item a query
    cfg5  N = 1 000 000, d = 256 (one GPU's catalogue), a 131 072-row sample of the items as queries

Per metric: five alternating repeats of each path after one warm-up of each (device events around the whole call, the
host waits on the last event), median and spread (max - min) of each, query items/s, and 2 Q C d / time as a fraction of
the 2.5 PFLOP/s bf16 peak -- an end-to-end rate over peak (selection, epilogue and launch gaps included), not a
kernel's share of peak.  Needs a GPU; there is no CPU path.  One process per shape: run the shapes as separate commands,
each under its own time limit."""
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

SHAPES = {"cfg3": (100_000, 128, None), "cfg5": (1_000_000, 256, 131_072), "tiny": (5_000, 64, 1_024)}
METRICS = ("dot_product", "cosine_similarity", "euclidean_distance_sim")
PEAK_BF16 = 2.5e15


def table(n, d, seed=0):
    """trained-like rows: a rank-16 part plus noise (the generator of tests/test_gpu_item_knn.py), in chunks on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    G2 = torch.randn(16, d, generator=g, device="cuda")
    out = torch.empty((n, d), dtype=torch.float32, device="cuda")
    for lo in range(0, n, 65536):
        hi = min(n, lo + 65536)
        out[lo:hi] = 0.05 * torch.randn(hi - lo, 16, generator=g, device="cuda") @ G2 + \
            0.1 * torch.randn(hi - lo, d, generator=g, device="cuda")
    return out


def torch_baseline(E_b, norms, query, k, metric, chunk):
    """materialise-and-topk: bf16 matmul with fp32 output where torch offers it (else the bf16 product widened), the
    epilogue in the normative operation order, the query's own column removed, torch.topk"""
    n = E_b.shape[0]
    idx = torch.empty((query.numel(), k), dtype=torch.int64, device=E_b.device)
    val = torch.empty((query.numel(), k), dtype=torch.float32, device=E_b.device)
    Et = E_b.t()
    sq = torch.sqrt(norms)
    for lo in range(0, query.numel(), chunk):
        q = query[lo: lo + chunk].long()
        try:
            S = torch.mm(E_b[q], Et, out_dtype=torch.float32)
        except TypeError:
            S = torch.mm(E_b[q], Et).float()
        if metric == "cosine_similarity":
            S = S / (sq[q][:, None] * sq[None, :])
            S = torch.where(torch.isfinite(S), S, torch.full_like(S, float("-inf")))
        elif metric == "euclidean_distance_sim":
            S = 1.0 / (1.0 + torch.sqrt(torch.clamp_min((norms[q][:, None] + norms[None, :]) - 2.0 * S, 0.0)))
        S[torch.arange(q.numel(), device=S.device), q] = float("-inf")
        v, i = torch.topk(S, k, dim=1)
        idx[lo: lo + chunk], val[lo: lo + chunk] = i, v
        del S
    return idx, val


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
    ap.add_argument("--metric", nargs="*", default=list(METRICS), choices=METRICS)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-chunk", type=int, default=None)
    ap.add_argument("--out", default=None, help="JSON file to merge this shape's result into")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd.core import CQLCore, CQLHyper
    n, d, nq = SHAPES[args.shape]
    core = CQLCore(n, CQLHyper(d=d), device="cuda:0")
    core.segment(core.theta, "E_out").copy_(table(n, d))
    core.refresh_shadows()
    E_b = core.segment(core.theta_b, "E_out")
    norms = core.item_norms()
    if nq is None:
        query = torch.arange(n, dtype=torch.int32, device="cuda")
    else:
        query = torch.sort(torch.randperm(n, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")[:nq])[0].int()
    Q = query.numel()
    bchunk = args.baseline_chunk or max(256, min(8192, (4 << 30) // (4 * n)))    # 4 GiB of fp32 scores per chunk
    flop = 2.0 * Q * n * d
    result = {"shape": args.shape, "n_items": n, "d": d, "queries": Q, "k": args.k, "repeats": args.repeats,
              "baseline_chunk": bchunk, "device": torch.cuda.get_device_name(0), "metrics": {}}
    for metric in args.metric:
        new = lambda: core.item_knn(query, args.k, metric)                        # noqa: E731
        old = lambda: torch_baseline(E_b, norms, query, args.k, metric, bchunk)   # noqa: E731
        (_, (ni, nv, _)), (_, (bi, _)) = timed(new), timed(old)                    # warm-up of both + agreement
        agree = float((torch.sort(ni.long(), 1)[0] == torch.sort(bi, 1)[0]).float().mean())
        t_new, t_old = [], []
        for _ in range(args.repeats):                                              # alternating
            t_new.append(timed(new)[0])
            t_old.append(timed(old)[0])
        m_new, m_old = statistics.median(t_new), statistics.median(t_old)
        s_new, s_old = max(t_new) - min(t_new), max(t_old) - min(t_old)
        row = {"new_s": t_new, "baseline_s": t_old, "new_median_s": m_new, "baseline_median_s": m_old,
               "new_spread_s": s_new, "baseline_spread_s": s_old, "query_items_per_s": Q / m_new,
               "baseline_query_items_per_s": Q / m_old, "fraction_of_bf16_peak": flop / m_new / PEAK_BF16,
               "baseline_fraction_of_bf16_peak": flop / m_old / PEAK_BF16, "speedup": m_old / m_new,
               "faster_by_more_than_the_spreads": bool(min(t_old) - max(t_new) > 0 and m_old - m_new > s_new + s_old),
               "neighbour_slots_equal_to_baseline": agree}
        result["metrics"][metric] = row
        print(json.dumps({"shape": args.shape, "metric": metric, **{k_: v for k_, v in row.items() if not k_.endswith("_s") or "median" in k_ or "spread" in k_}}), flush=True)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        blob = json.loads(path.read_text()) if path.exists() else {}
        blob[args.shape] = result
        path.write_text(json.dumps(blob, indent=1) + "\n")


if __name__ == "__main__":
    main()
