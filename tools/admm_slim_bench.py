"""Times ADMM SLIM (replay_cql_amd.admm_slim -> section f11, csrc/dense.hip) and the fp64 GEMM under it.

    python tools/admm_slim_bench.py [--gemm-sizes 4096 8192 16384] [--fit-items 8192 16384] [--repeats 5]
                                    [--out profiles/admm_slim_bench.json]

Each number is the median of `repeats` whole calls after one warm-up (host clock around a call that ends in a device
synchronise), with the spread (max - min):
  gemm n               cqlrec_dense_gemm_f64 on two random n x n matrices, beside torch.matmul in fp64 on the same matrices in
                       the same process, the two sides alternating call by call; TFLOP/s = 2 n^3 / time, beside the 78.6
                       TFLOP/s of the fp64 VECTOR peak (nobody has published the matrix figure of this chip)
  per item count n     the cfg3 log (tools/bench_record.make_log: 1 M users, 100 000 items, about 48 M rows) cut to its n most
                       frequent items with the package's own filter_by_min_count and Indexer; then
                       ADMMSLIM().fit (the defaults lambda_1 = 5, lambda_2 = 5000, seed 0), with its iteration count;
                       one cqlrec_admm_iteration alone on the fitted W and P; cqlrec_dense_spd_inverse alone;
                       the Gram matrix alone; recommend(k = 10) for every user of the cut log
                       and the GEMM alone on the n_items of the cut log (ties at the cut add a few items to n)
At the end the two relations the arithmetic predicts: iteration / GEMM on the same shape (about 1: an iteration adds
O(n^2) work to its GEMM) and inverse / iteration (two to three).  Needs a GPU."""
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

from tools.bench_record import Recorder, make_log, timed, repeat as bench_repeat          # noqa: E402  pylint: disable=wrong-import-position

FP64_VECTOR_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--gemm-sizes", type=int, nargs="*", default=[4096, 8192, 16384])
    ap.add_argument("--fit-items", type=int, nargs="*", default=[8192, 16384])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--max-recommend-tuples", type=float, default=2e11,
                    help="recommend is skipped, and said to be, when its sparse product expands beyond this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("admm_slim_bench needs a GPU: a CPU run gives no time")
    from replay_cql_amd import admm_slim as AS
    from replay_cql_amd._dense import Dense
    from replay_cql_amd.filters import filter_by_min_count
    from replay_cql_amd.indexer import Indexer
    dev = torch.device("cuda:0")
    D = Dense(dev)
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "fp64_vector_peak_tflops": FP64_VECTOR_PEAK_TFLOPS,
              "calls": {}}

    rec = Recorder(result, args.out)
    record, save = rec.record, rec.save

    def repeat(fn):
        return bench_repeat(fn, args.repeats)

    # ---- the GEMM alone, beside torch.matmul --------------------------------------------------------------------
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in args.gemm_sizes:
        A = torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen)
        Bm = torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen)
        out = torch.empty_like(A)
        timed(lambda: D.gemm(A, Bm, out=out))
        timed(lambda: torch.matmul(A, Bm, out=out))
        ours, theirs = [], []
        for _ in range(args.repeats):                       # the sides alternate
            ours.append(timed(lambda: D.gemm(A, Bm, out=out))[0])
            theirs.append(timed(lambda: torch.matmul(A, Bm, out=out))[0])
        flop = 2.0 * n ** 3
        a = record(f"dense_gemm_f64 n={n}", ours, tflops=flop / statistics.median(ours) / 1e12,
                   of_fp64_vector_peak=flop / statistics.median(ours) / 1e12 / FP64_VECTOR_PEAK_TFLOPS)
        b = record(f"torch.matmul fp64 n={n}", theirs, tflops=flop / statistics.median(theirs) / 1e12)
        result.setdefault("ratios", {})[f"torch_matmul_time_over_dense_gemm_time n={n}"] = b / a
        del A, Bm, out
    save()

    # ---- the model on the cut cfg3 log -----------------------------------------------------------------------------
    if args.fit_items:
        log = make_log(args.users, args.items, dev)
        counts = torch.bincount(log["item_idx"].long(), minlength=args.items)
        ranked = torch.sort(counts, descending=True).values
    for n in args.fit_items:
        threshold = int(ranked[n - 1].item())               # the count of the n-th most frequent item: ties may add a few
        cut = filter_by_min_count(log, threshold, "item_idx")
        raw = {"user_id": cut["user_idx"], "item_id": cut["item_idx"], "relevance": cut["relevance"]}
        indexer = Indexer()
        indexer.fit(raw, raw)
        small = indexer.transform(raw)
        n_items = int(small["item_idx"].max().item()) + 1
        n_users = int(small["user_idx"].max().item()) + 1
        shape = {"items": n_items, "users": n_users, "rows": int(small["item_idx"].numel()), "min_count": threshold}

        def fit():
            m = AS.ADMMSLIM(seed=0)
            m.fit(small)
            return m
        times, model = repeat(fit)
        fit_s = record(f"ADMMSLIM().fit items={n}", times, iterations=model.n_iterations, rho=model.rho,
                       table_nnz=int(model.similarity_device[1].numel()), **shape)

        # the pieces, on the matrices of this log
        item, user = small["item_idx"], small["user_idx"]
        rel = small["relevance"].to(torch.float64)
        views = (D.view(item, n_items, user, rel)[0], D.view(user, n_users, item, rel)[0])
        times, G = repeat(lambda: D.gram(*views, n_items, n_users))
        record(f"dense_gram items={n}", times, **shape)
        del views
        times, W = repeat(lambda: D.spd_inverse(G, 2.0 * model.lambda_2))
        inv_s = record(f"dense_spd_inverse items={n}", times, tflops_of_3n3=3.0 * n_items ** 3 / statistics.median(times) / 1e12)
        Pm = D.gemm(W, G)
        del G
        C = torch.rand((n_items, n_items), dtype=torch.float64, device=dev, generator=gen)
        Gamma = torch.rand((n_items, n_items), dtype=torch.float64, device=dev, generator=gen)
        ws, sums = D._ws(D.ws_bytes("admm_iteration", n_items)), D._empty(5, torch.float64)
        times, _ = repeat(lambda: D.admm_iteration(W, Pm, C, Gamma, float(model.lambda_2), float(model.lambda_1), ws, sums))
        it_s = record(f"admm_iteration items={n}", times, tflops=2.0 * n_items ** 3 / statistics.median(times) / 1e12)
        times, _ = repeat(lambda: D.gemm(W, Pm, out=C))      # the GEMM alone on this very shape: a cut at a tie is not n
        gemm_s = record(f"dense_gemm_f64 items={n}", times, n=n_items, tflops=2.0 * n_items ** 3 / statistics.median(times) / 1e12)
        del W, Pm, C, Gamma, ws
        ratios = result.setdefault("ratios", {})
        ratios[f"admm_iteration_over_dense_gemm items={n}"] = it_s / gemm_s
        ratios[f"spd_inverse_over_admm_iteration items={n}"] = inv_s / it_s
        ratios[f"fit_minus_iterations_s items={n}"] = fit_s - model.n_iterations * it_s

        off = model.similarity_device[0]
        row_nnz = (off[1:] - off[:-1])
        tuples = int(row_nnz[item.long()].sum().item())
        if tuples <= args.max_recommend_tuples:
            times, out = repeat(lambda: model.recommend(small, args.k))
            record(f"ADMMSLIM.recommend(all users, k={args.k}) items={n}", times, expansion_tuples=tuples,
                   rows_out=int(out["item_idx"].numel()), users_per_s=n_users / statistics.median(times))
            del out
        else:
            result["calls"][f"ADMMSLIM.recommend(all users, k={args.k}) items={n}"] = {
                "skipped": f"the sparse product of the log with the table expands to {tuples} tuples, beyond --max-recommend-tuples"}
        del model, small, cut, raw
        save()
    print(json.dumps({"ratios": result.get("ratios", {})}), flush=True)
    save()


if __name__ == "__main__":
    main()
