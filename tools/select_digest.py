#!/usr/bin/env python3
"""SHA-256 of what the selection kernels outside the predict pass return, on fixed seeds -- for bit-for-bit A/B runs of
two builds in separate processes (CQLREC_LIB selects the library), beside tools/topk_digest.py:

    knn    CQLCore.item_knn: ITEMS items (d = 64), every item a query, the three metrics, k = 10 and 100
    pairs  CQLCore.pairs_topk: ROWS rows of 600 candidates drawn from 60 ids (each listed several times: the equal-key
           case of the shared select), a seen list per row, k = 10

    python tools/select_digest.py [--items 3000] [--rows 300]
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from replay_cql_amd.core import CQLCore, CQLHyper  # noqa: E402


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=3000)
    ap.add_argument("--rows", type=int, default=300)
    a = ap.parse_args()
    n, d = a.items, 64
    g = torch.Generator().manual_seed(20240607)
    core = CQLCore(n, CQLHyper(d=d), device="cuda:0")
    core.segment(core.theta, "E_out").copy_((0.1 * torch.randn(n, d, generator=g)).cuda())   # distinct rows
    core.refresh_shadows()
    out = {}
    q = torch.arange(n, dtype=torch.int32, device="cuda")
    for metric in ("dot_product", "cosine_similarity", "euclidean_distance_sim"):
        for k in (10, 100):
            out[f"knn {metric} k={k}"] = digest(*core.item_knn(q, k, metric))
    per, pool = 600, 60
    items = torch.sort(torch.randint(0, pool, (a.rows, per), generator=g) * (n // pool), dim=1)[0].to(torch.int32).cuda()
    off = torch.arange(a.rows + 1, dtype=torch.int64, device="cuda") * per
    seen_items = (torch.arange(0, pool, 7, dtype=torch.int32) * (n // pool)).repeat(a.rows).cuda()
    seen_off = torch.arange(a.rows + 1, dtype=torch.int64, device="cuda") * len(range(0, pool, 7))
    hb = torch.randn(a.rows, d, generator=g).to(torch.bfloat16).cuda()
    idx, val, cnt = core.pairs_topk(hb, off, items.view(-1), None, 10, seen=(seen_off, seen_items))
    out["pairs k=10"] = digest(idx, val, cnt)
    out["pairs cnt_min"] = int(cnt.min())
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
