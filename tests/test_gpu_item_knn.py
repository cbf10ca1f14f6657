"""Item-to-item nearest neighbours on the GPU (cqlrec_item_knn and everything above it) against tests/knn_reference.py.

Exactness (P2).  Tables with entries on the 2^-6 grid, |x| <= 2: every product lies on the 2^-12 grid, every dot, norm
and (n_i + n_j) - 2 dot has |sum| <= 4096 there = 24 bits, so fp32 accumulates them without rounding in any order and
the remaining operations (sqrt, *, /, +, max) are correctly rounded on both sides: ids AND value bits must equal the
float32 evaluation of the reference.

Random tables (P3-style): values are compared with float64 under a per-pair bound that is derived, not tuned.  With
u = 2^-24 (fp32 unit roundoff), products of bf16 values exact and gamma = d u / (1 - d u) (any summation order):
    dot      |dot_hat - dot| <= gamma S,                     S = sum_t |v_i[t] v_j[t]|
    norms    n_hat = n (1 + th), |th| <= gamma
    cosine   sqrt halves the relative error of n_hat and adds u (x2), the product of the roots adds u, the division u:
             relative error of the denominator <= gamma + 3u + O(u^2), of the quotient one more u; the numerator's
             absolute error gamma S divided by the denominator.  With |dot| <= S:
             |cos_hat - cos| <= (2 gamma + 6u) S / (|v_i| |v_j|)           (the 6u leaves room for the O(u^2) terms)
    euclid   x = (n_i + n_j) - 2 dot: the norms carry gamma (n_i + n_j), the sum one rounding u (n_i + n_j), the
             difference one rounding u |x| <= u (n_i + n_j + 2S), 2 dot carries 2 gamma S (doubling is exact):
             |x_hat - x| <= (gamma + 3u) (n_i + n_j + 2S) =: dx;  f(x) = 1/(1 + sqrt(max(x, 0))) is non-increasing and
             convex on x >= 0, so |f(x_hat) - f(x)| <= f(max(x - dx, 0)) - f(x); sqrt, +, / add at most 4u (f <= 1).
Neighbour sets must be equal once the neighbours whose float64 value lies within twice that bound of the row's k-th
value are left out (and, in a row that has one, the k-th itself: it may trade places with it).  At most 10 % of the
query rows may have any neighbour left out and at most 2 % of all Q k neighbour slots; both shares are asserted for the
reference alone first."""
import numpy as np
import pandas as pd
import pytest
import torch

import knn_reference as R
from helpers import bf16_dev, dev, ptr, stream, sync
from replay_cql_amd import _native as N

pytestmark = pytest.mark.gpu

METRIC_ID = {"dot_product": N.SIM_DOT, "cosine_similarity": N.SIM_COSINE, "euclidean_distance_sim": N.SIM_EUCLID}
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    return N.load()


def run_abi(lib, E_b, query, cand, metric, k, norms=None):
    """one cqlrec_item_norms + cqlrec_item_knn call; returns numpy (idx, val, cnt)"""
    n_rows, d = E_b.shape
    if norms is None:
        norms = torch.empty(n_rows, dtype=torch.float32, device="cuda")
        N.check(lib.cqlrec_item_norms(ptr(E_b), n_rows, d, ptr(norms), stream()), "item_norms")
    q = dev(np.asarray(query, dtype=np.int32))
    c = None if cand is None else dev(np.asarray(cand, dtype=np.int32))
    n_cand = n_rows if c is None else c.numel()
    wsb = lib.cqlrec_item_knn_ws_bytes(q.numel(), n_cand, d, k)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    idx = torch.full((q.numel(), k), -7, dtype=torch.int32, device="cuda")
    val = torch.full((q.numel(), k), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((q.numel(),), -7, dtype=torch.int32, device="cuda")
    N.check(lib.cqlrec_item_knn(ptr(E_b), ptr(norms), n_rows, d, ptr(q), q.numel(), ptr(c), n_cand, METRIC_ID[metric], k,
                                ptr(ws), wsb, ptr(idx), ptr(val), ptr(cnt), stream()), "item_knn")
    sync()
    return idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()


def grid_table(n, d, seed):
    """2^-6 grid, |x| <= 2; every 7th row of the upper half repeats a row of the lower half; one all-zero row"""
    rng = np.random.default_rng(seed)
    V = rng.integers(-128, 129, size=(n, d)).astype(np.float32) / 64.0
    dup = np.arange(n // 2, n, 7)
    V[dup] = V[rng.integers(0, n // 2, size=len(dup))]
    zero = n // 3
    V[zero] = 0.0
    return V, dup, zero


@pytest.mark.parametrize("n", [10007, 66000])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_exact_on_grid_tables(lib, n, d):
    V, dup, zero = grid_table(n, d, seed=n + d)
    E_b = bf16_dev(V)
    rng = np.random.default_rng(5)
    query = np.concatenate([[zero], dup[:40], rng.choice(n, 90, replace=False)])
    query = rng.permutation(np.unique(query))
    subset = rng.permutation(np.unique(np.concatenate([rng.choice(n, n // 2, replace=False), dup[:200], [zero]])))
    norms = torch.empty(n, dtype=torch.float32, device="cuda")
    N.check(lib.cqlrec_item_norms(ptr(E_b), n, d, ptr(norms), stream()), "item_norms")
    sync()
    assert np.array_equal(norms.cpu().numpy(), (V * V).sum(axis=1, dtype=np.float32))
    for metric in R.METRICS:
        for cand in (None, subset):
            cids = np.arange(n) if cand is None else cand
            ridx, rval, rcnt = R.nearest_items(V, query, cids, 512, metric, dtype=np.float32)
            assert rval.dtype == np.float32
            for k in (1, 10, 100, 512):
                idx, val, cnt = run_abi(lib, E_b, query, cand, metric, k, norms)
                what = f"n={n} d={d} {metric} k={k} subset={cand is not None}"
                assert np.array_equal(cnt, np.minimum(rcnt, k)), what
                assert np.array_equal(idx, ridx[:, :k]), what
                assert np.array_equal(val.view(np.uint32), rval[:, :k].view(np.uint32)), what
            zq = int(np.where(query == zero)[0][0])
            if metric == "cosine_similarity":
                assert rcnt[zq] == 0                              # every denominator of the zero row is 0
            assert not np.any(ridx == query[:, None])             # the reference itself: never its own neighbour


def test_k_at_the_limit_keeps_exactly_k(lib):
    """k = 512 = KNN_MAX_K over 2 048 candidates (64 groups, tg = 1): every tighten has to leave exactly k survivors,
    half of the 1 024-entry buffer, and all k output slots are filled.  At this shape the slack tighten fires at
    k + k / 8 = 576 keys, so the buffer-full branch (reached only with tg >= 16) is not what this pins.  Dot product on
    the grid table: ids and value bits of the reference."""
    n, d, k = 2048, 64, 512
    V, dup, zero = grid_table(n, d, seed=77)
    query = np.unique(np.concatenate([[zero], dup[:8], np.arange(0, n, 97)]))
    ridx, rval, rcnt = R.nearest_items(V, query, np.arange(n), k, "dot_product", dtype=np.float32)
    idx, val, cnt = run_abi(lib, bf16_dev(V), query, None, "dot_product", k)
    assert np.array_equal(cnt, rcnt) and np.all(cnt == k)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(val.view(np.uint32), rval.view(np.uint32))


def trained_like(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    G1, G2, G3 = torch.randn(n, 16, generator=g), torch.randn(16, d, generator=g), torch.randn(n, d, generator=g)
    return (0.05 * G1 @ G2 + 0.1 * G3).to(torch.bfloat16).to(torch.float32).numpy()


def pair_bound(V64, q, c, metric, d):
    """the per-pair error bound of the module docstring, [len(q) x len(c)] float64"""
    gam = d * U32 / (1 - d * U32)
    A = np.abs(V64)
    S = A[q] @ A[c].T
    n = (V64 * V64).sum(axis=1)
    if metric == "dot_product":
        return gam * S
    if metric == "cosine_similarity":
        with np.errstate(divide="ignore", invalid="ignore"):
            return (2 * gam + 6 * U32) * S / (np.sqrt(n[q])[:, None] * np.sqrt(n[c])[None, :])
    x = np.maximum((n[q][:, None] + n[c][None, :]) - 2 * (V64[q] @ V64[c].T), 0)
    dx = (gam + 3 * U32) * (n[q][:, None] + n[c][None, :] + 2 * S)
    f = lambda t: 1 / (1 + np.sqrt(t))      # noqa: E731
    return f(np.maximum(x - dx, 0)) - f(x) + 4 * U32


def check_against_float64(V, query, idx, val, cnt, metric, k, d):
    """values within the bound; neighbour sets equal outside the margin; the two caps hold for the reference alone"""
    n = V.shape[0]
    V64, cids = V.astype(np.float64), np.arange(n)
    v64, ok = R.pair_values(V64, query, cids, metric)
    bnd = pair_bound(V64, query, cids, metric, d)
    ridx, rval, rcnt = R.nearest_items(V64, query, cids, k, metric)
    assert np.all(rcnt == k)
    Q = len(query)
    kth_val, kth_id = rval[:, k - 1], ridx[:, k - 1]
    near = ok & (np.abs(v64 - kth_val[:, None]) <= 2 * bnd)
    near[np.arange(Q), kth_id] = False                      # the k-th itself is not counted
    rows_share, slots_share = near.any(axis=1).mean(), near.sum() / (Q * k)
    print(f"{metric} d={d}: rows with a boundary neighbour {rows_share:.4f}, slots {slots_share:.4f}")
    assert rows_share <= 0.10 and slots_share <= 0.02, "the reference alone breaks the caps on these inputs"
    assert np.array_equal(cnt, rcnt)
    worst = 0.0
    for r in range(Q):
        got = idx[r]
        assert np.all(ok[r, got]) and len(set(got.tolist())) == k
        err = np.abs(val[r].astype(np.float64) - v64[r, got])
        worst = max(worst, float(np.max(err / bnd[r, got])))
        assert np.all(err <= bnd[r, got]), (metric, d, r, err, bnd[r, got])
        # order inside the row: value descending, equal values id descending
        assert np.all(np.diff(val[r]) <= 0) and np.all((np.diff(val[r]) < 0) | (np.diff(got) < 0))
        left = set(np.where(near[r])[0].tolist())
        if left:
            left.add(int(kth_id[r]))
        assert set(got.tolist()) - left == set(ridx[r].tolist()) - left, (metric, d, r)
    print(f"{metric} d={d}: largest |value - float64| / bound = {worst:.3f}")


@pytest.mark.parametrize("d", [64, 128, 256])
def test_random_tables_within_the_derived_bound(lib, d):
    n, Q, k = 20000, 2048, 10
    V = trained_like(n, d, seed=100 + d)
    E_b = bf16_dev(V)
    query = np.random.default_rng(d).choice(n, Q, replace=False)
    for metric in R.METRICS:
        idx, val, cnt = run_abi(lib, E_b, query, None, metric, k)
        check_against_float64(V, query, idx, val, cnt, metric, k, d)


def test_full_size_cosine_sample(lib):
    """the timed shape: 100 000 items, d = 128, every item a query, k = 10; a 4 096-row sample checked as above"""
    from replay_cql_amd.core import CQLCore, CQLHyper
    n, d, k = 100000, 128, 10
    V = trained_like(n, d, seed=9)
    core = CQLCore(n, CQLHyper(d=d), device="cuda:0")
    core.segment(core.theta, "E_out").copy_(torch.from_numpy(V).cuda())
    core.refresh_shadows()
    idx, val, cnt = core.item_knn(torch.arange(n, dtype=torch.int32, device="cuda"), k, "cosine_similarity")
    sync()
    rows = np.sort(np.random.default_rng(1).choice(n, 4096, replace=False))
    check_against_float64(V, rows, idx.cpu().numpy()[rows], val.cpu().numpy()[rows], cnt.cpu().numpy()[rows],
                          "cosine_similarity", k, d)


U_, NI, D_ = 90, 300, 64


@pytest.fixture(scope="module")
def fitted():
    from oracle import cql_oracle as O
    from replay_cql_amd.cql import CQL
    u, i, t, r = O.synth_log(U_, NI, seed=4, mean_len=12, max_len=30)
    log = pd.DataFrame({"user_idx": u, "item_idx": i, "timestamp": pd.to_datetime(t, unit="s"), "relevance": r})
    log = log[log.item_idx % 11 != 3]                  # some rows below the catalogue size were never seen at fit
    m = CQL(embedding_dim=D_, window=8, batch_size=64, n_steps=6, seed=3, device="cuda:0")
    m.fit(log)
    return m


def _frame_of(ridx, rval, rcnt, query, metric):
    rows = [(int(q), int(ridx[r, j]), float(rval[r, j])) for r, q in enumerate(query) for j in range(int(rcnt[r]))]
    return pd.DataFrame(rows, columns=["item_idx", "neighbour_item_idx", metric]).astype(
        {"item_idx": np.int32, "neighbour_item_idx": np.int32, metric: np.float64})


@pytest.mark.parametrize("metric", R.METRICS)
def test_same_answer_through_every_layer(lib, fitted, tmp_path, metric):
    from replay_cql_amd import torch_ops
    from replay_cql_amd.cql import CQL
    m, k = fitted, 5
    core = m.core
    E_b = core.segment(core.theta_b, "E_out").contiguous()
    V = E_b.to(torch.float32).cpu().numpy()
    fit_items = np.sort(m.fit_items["item_idx"].to_numpy().astype(np.int64))
    assert len(fit_items) < core.n_items
    unseen = int(np.setdiff1d(np.arange(core.n_items), fit_items)[0])
    items = [int(fit_items[5]), int(fit_items[0]), unseen, int(fit_items[5]), int(fit_items[-1])]
    query = np.array([fit_items[0], fit_items[5], fit_items[-1]])          # ascending: the order the frames come in
    ridx, rval, rcnt = R.nearest_items(V, query, fit_items, k, metric, dtype=np.float64)
    want = _frame_of(ridx, rval, rcnt, query, metric)

    def same(frame):
        frame = frame.reset_index(drop=True)
        assert list(frame.columns) == ["item_idx", "neighbour_item_idx", metric]
        assert frame["item_idx"].dtype == np.int32 and frame["neighbour_item_idx"].dtype == np.int32
        assert frame[metric].dtype == np.float64
        assert frame[["item_idx", "neighbour_item_idx"]].equals(want[["item_idx", "neighbour_item_idx"]])
        np.testing.assert_allclose(frame[metric], want[metric], rtol=1e-5, atol=1e-6)

    a = m.get_nearest_items(items, k, metric)
    same(a)
    b = m.get_nearest_items(items, k, metric)
    assert a.equals(b)                                                       # two calls: identical bits
    rb = m.nearest_items_arrow(items, k, metric)
    assert rb.schema.names == ["item_idx", "neighbour_item_idx", metric]
    assert rb.to_pandas().equals(a)
    # the C ABI and the torch operator on the same rows
    idx, val, cnt = run_abi(lib, E_b, query, fit_items, metric, k)
    got = _frame_of(idx, val, cnt, query, metric)
    assert got.equals(a.reset_index(drop=True))
    ops = torch_ops.load()
    ti, tv, tc = ops.item_knn(E_b, dev(query.astype(np.int32)), k, METRIC_ID[metric], dev(fit_items.astype(np.int32)), None)
    assert np.array_equal(ti.cpu().numpy(), idx) and np.array_equal(tc.cpu().numpy(), cnt)
    assert np.array_equal(tv.cpu().numpy().view(np.uint32), val.view(np.uint32))
    # query chunking does not change the result
    allq = torch.as_tensor(fit_items.astype(np.int32)).cuda()
    one = core.item_knn(allq, k, metric, cand_ids=allq)
    many = core.item_knn(allq, k, metric, cand_ids=allq, chunk=37)
    for x, y in zip(one, many):
        assert torch.equal(x, y)
    # candidates: ids not seen at fit are dropped; k above the candidate count is clamped
    cands = [int(fit_items[1]), unseen, int(fit_items[5]), int(fit_items[9])]
    c = m.get_nearest_items([int(fit_items[5])], 50, metric, candidates=cands)
    assert sorted(c["neighbour_item_idx"]) == sorted([int(fit_items[1]), int(fit_items[9])])
    # after save / load
    path = str(tmp_path / "cql.pt")
    m._save_model(path)
    m2 = CQL(embedding_dim=D_, device="cuda:0")
    m2._load_model(path)
    assert m2.get_nearest_items(items, k, metric).equals(a)
    assert m2.nearest_items_arrow(items, k, metric).to_pandas().equals(a)


def test_errors(fitted):
    with pytest.raises(NotImplementedError, match="euclidean_distance_sim"):
        fitted.get_nearest_items([1], 3, "manhattan")
    with pytest.raises(ValueError):
        fitted.get_nearest_items([1], 3, None)
    from replay_cql_amd.core import CQLCore, CQLHyper
    allq = torch.arange(fitted.core.n_items, dtype=torch.int32, device="cuda")
    idx, _, cnt = fitted.core.item_knn(allq, 600, "dot_product")          # k is clamped to the number of candidates
    assert idx.shape == (fitted.core.n_items, fitted.core.n_items) and int(cnt.min()) == fitted.core.n_items - 1
    big = CQLCore(1000, CQLHyper(d=64), device="cuda:0")
    with pytest.raises(ValueError, match="512"):
        big.item_knn(allq, 600, "dot_product")
    with pytest.raises(ValueError, match="item ids"):
        big.item_knn(torch.tensor([1000], dtype=torch.int32), 5, "dot_product")
