"""CPU checks of tests/pairs_reference.py, the statement the candidate-list kernels are compared with: its ranking is
`recommender_api.get_top_k` (what predict_pairs(k=) applies on the host), duplicates stay, the seen anti-join, the score
emulation against a float64 dot, and the arithmetic evaluate_candidates performs against tests/metrics_reference.py."""
import numpy as np
import pandas as pd
import pytest

import metrics_reference as MR
import pairs_reference as PR
from oracle import cql_oracle as O
from replay_cql_amd.recommender_api import get_top_k


def _frame(rng, n_users, max_len, n_items, levels=None):
    rows = []
    for u in range(n_users):
        n = int(rng.integers(0, max_len + 1))
        it = rng.integers(0, n_items, n)
        sc = rng.standard_normal(n).astype(np.float32) if levels is None else rng.integers(0, levels, n).astype(np.float32)
        rows += [(u, int(i), float(s)) for i, s in zip(it, sc)]
    return pd.DataFrame(rows, columns=["user_idx", "item_idx", "relevance"])


@pytest.mark.parametrize("levels", [None, 3])
@pytest.mark.parametrize("k", [1, 4, 50])
def test_ranking_equals_get_top_k(levels, k):
    rng = np.random.default_rng(11 + k)
    df = _frame(rng, 40, 30, 12 if levels else 500, levels)        # few items + few score levels: ties and duplicates
    exp = get_top_k(df, "user_idx", [("relevance", False), ("item_idx", True)], k).reset_index(drop=True)
    srt = df.sort_values(["user_idx", "item_idx"], kind="stable")
    off = np.zeros(41, np.int64)
    np.cumsum(np.bincount(srt.user_idx, minlength=40), out=off[1:])
    idx, val, cnt = PR.rank_lists(off, srt.item_idx.to_numpy(), srt.relevance.to_numpy(np.float32), np.arange(40), k)
    got = pd.DataFrame({"user_idx": np.repeat(np.arange(40), cnt), "item_idx": idx[idx >= 0].astype(np.int64),
                        "relevance": val[idx >= 0].astype(np.float64)})
    assert cnt.tolist() == [min(k, n) for n in np.diff(off)]
    pd.testing.assert_frame_equal(got, exp[["user_idx", "item_idx", "relevance"]], check_dtype=False)


def test_duplicates_are_kept_and_adjacent():
    it, sc = PR.rank_list([3, 3, 5, 5, 5, 9], np.float32([2, 2, 2, 2, 2, 7]), 4)
    assert it.tolist() == [9, 3, 3, 5] and sc.tolist() == [7, 2, 2, 2]
    it, _ = PR.rank_list([3, 3, 5, 5, 5, 9], np.float32([2, 2, 2, 2, 2, 7]), 10)
    assert it.tolist() == [9, 3, 3, 5, 5, 5]


def test_seen_anti_join():
    it, sc = PR.rank_list([1, 2, 2, 4], np.float32([1, 5, 5, 3]), 3, seen=[2, 7])
    assert it.tolist() == [4, 1] and sc.tolist() == [3, 1]
    assert PR.rank_list([1, 2], np.float32([1, 2]), 3, seen=[1, 2])[0].size == 0
    assert PR.rank_list([1, 2], np.float32([1, 2]), 3, seen=[])[0].tolist() == [2, 1]
    off, items = PR.csr_of_lists({0: [4, 1, 1], 2: [7]}, 3)
    assert off.tolist() == [0, 3, 3, 4] and items.tolist() == [1, 1, 4, 7]


@pytest.mark.parametrize("d", [64, 128, 256])
def test_score_emulation(d):
    rng = np.random.default_rng(d)
    # dyadic values: every partial sum is exact, so any summation order gives the float64 dot
    h = O.bf16_bits((rng.integers(-4, 5, (5, d)) / 4).astype(np.float32))
    e = O.bf16_bits((rng.integers(-4, 5, (30, d)) / 8).astype(np.float32))
    b = (rng.integers(-8, 9, 30) / 16).astype(np.float32)
    row, item = rng.integers(0, 5, 200), rng.integers(0, 30, 200)
    got = PR.gather_dot(h, e, b, row, item)
    hf, ef = PR.bf16_bits_to_f32(h).astype(np.float64), PR.bf16_bits_to_f32(e).astype(np.float64)
    assert got.dtype == np.float32 and np.array_equal(got, (np.einsum("pd,pd->p", hf[row], ef[item]) + b[item]))
    # random values: float32 rounding per step; within n_terms * eps * sum|terms| of the float64 dot
    h = O.bf16_bits(rng.standard_normal((5, d)).astype(np.float32))
    e = O.bf16_bits(rng.standard_normal((30, d)).astype(np.float32))
    got = PR.gather_dot(h, e, b, row, item)
    hf, ef = PR.bf16_bits_to_f32(h).astype(np.float64), PR.bf16_bits_to_f32(e).astype(np.float64)
    bound = (d + 1) * 2.0 ** -24 * (np.abs(hf[row] * ef[item]).sum(1) + np.abs(b[item]))
    assert np.all(np.abs(got - (np.einsum("pd,pd->p", hf[row], ef[item]) + b[item])) <= bound)


def test_evaluate_candidates_arithmetic():
    """evaluate_candidates = rank every user's candidates, then the metric definitions over the [n, max k] block with
    the users of the ground truth as rows; users without candidates count with empty predictions."""
    rng = np.random.default_rng(5)
    pairs = _frame(rng, 30, 25, 200).drop_duplicates(["user_idx", "item_idx"])
    gt = pd.DataFrame({"user_idx": rng.integers(0, 34, 120), "item_idx": rng.integers(0, 200, 120)}).drop_duplicates()
    ks = [1, 5, 10]
    gt_users = np.sort(gt.user_idx.unique())
    srt = pairs.sort_values(["user_idx", "item_idx"], kind="stable")
    off = np.zeros(35, np.int64)
    np.cumsum(np.bincount(srt.user_idx, minlength=34), out=off[1:])
    idx, _, _ = PR.rank_lists(off, srt.item_idx.to_numpy(), srt.relevance.to_numpy(np.float32), gt_users, 10)
    g_off = np.zeros(len(gt_users) + 1, np.int64)
    g = gt.sort_values(["user_idx", "item_idx"])
    np.cumsum(np.bincount(np.searchsorted(gt_users, g.user_idx), minlength=len(gt_users)), out=g_off[1:])
    from oracle import metrics_oracle as MO
    blk = MO.evaluate_block(idx, g_off, g.item_idx.to_numpy().astype(np.int32), ks)       # [users][6][ks]
    frame = list(pairs.itertuples(index=False, name=None))
    gt_rows = list(gt.itertuples(index=False, name=None))
    for mi, name in enumerate(("NDCG", "HitRate", "Precision", "Recall", "MAP", "MRR")):
        users, vals = MR.per_user_values(name, frame, ks, gt=gt_rows, gt_users=gt_users)
        for ki, k in enumerate(ks):
            assert blk[:, mi, ki].mean() == pytest.approx(MR.mean(vals[k]), rel=1e-12, abs=1e-15), (name, k)
