"""csrc/als.hip and replay_cql_amd.als on the GPU against the fsum yardstick (tests/als_reference.py): bit for bit on
dyadic inputs, within the derived bounds of `als_reference.tolerance` otherwise; the selection as a certificate.  Every
test prints its worst error / bound ratio (DESIGN.md section 3.10 records them)."""
import numpy as np
import pandas as pd
import pytest
import torch

import als_reference as R

pytestmark = pytest.mark.gpu

P = R.PIECE
RANKS = [1, 10, 33, 64, 128]
N_SRC = 50
CASE_ROWS = {"empty": 0, "one": 1, "nonpositive": 2, "duplicates": 3, "piece": 4, "piece+1": 5, "split": 6}


def dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dt is None else t.to(dt)


def eng():
    from replay_cql_amd.als import Als
    return Als(torch.device("cuda", torch.cuda.current_device()))


def make_side(seed, dyadic):
    """20 destination rows over 50 source rows: the seven cases of CASE_ROWS, then random short rows"""
    rng = np.random.default_rng(seed)

    def ratings(n):
        return rng.integers(-32, 33, n) / 4.0 if dyadic else np.round(rng.normal(size=n) * 3.0, 3)

    rows = [([], []), ([7], [2.5]), (rng.integers(0, N_SRC, 6), -np.abs(ratings(6)) * np.array([1, 1, 0, 1, 1, 0])),
            ([3, 3, 9, 3, 9, 12], [1.0, 0.5, -2.0, 1.0, 4.0, 0.25])]
    for n in (P, P + 1, 2 * P + 3):
        rows.append((rng.integers(0, N_SRC, n), ratings(n)))
    for n in rng.integers(2, 40, 13):
        rows.append((rng.choice(N_SRC, n, replace=False), np.abs(ratings(n)) + 0.25))
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r[0]) for r in rows])
    src = np.concatenate([np.asarray(r[0], dtype=np.int32) for r in rows]).astype(np.int32)
    rating = np.concatenate([np.asarray(r[1], dtype=np.float64) for r in rows])
    return off, src, rating


def make_factors(seed, rank, dyadic, n=N_SRC):
    rng = np.random.default_rng(seed)
    if dyadic:
        return (rng.integers(-128, 129, (n, rank)) / 64.0).astype(np.float32)
    F = rng.normal(size=(n, rank))
    return (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)


_cache = {}


def reference(rank, implicit, dyadic):
    """the yardstick's G, A, b, n_expl and sums of absolute terms, computed once per case"""
    key = (rank, implicit, dyadic)
    if key not in _cache:
        side, F = make_side(3, dyadic), make_factors(100 + rank, rank, dyadic)
        alpha = 0.5 if dyadic else 1.0
        gkey = ("G", rank, dyadic)
        if gkey not in _cache:
            _cache[gkey] = R.gram(F)
        G, Gs, g_exact = _cache[gkey]
        A, b, ne, SA, Sb, exact = R.normal_equations(side, F, implicit, alpha, G if implicit else None, Gs if implicit else None)
        _cache[key] = dict(side=side, F=F, alpha=alpha, G=G, Gs=Gs, A=A, b=b, ne=ne, SA=SA, Sb=Sb, exact=exact and g_exact)
    return _cache[key]


def ratio(err, tol):
    """the largest error / bound, an exact zero against a zero bound counting as 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(err > 0, err / tol, 0.0), initial=0.0))


def device_side(side):
    return dev(side[0]), dev(side[1]), dev(side[2])


def run_normal_equations(ref, implicit, rows=None):
    e = eng()
    F = dev(ref["F"])
    G = e.gram(F)
    A, b, ne = e.normal_equations(device_side(ref["side"]), F, G if implicit else None, implicit, ref["alpha"],
                                  rows=None if rows is None else dev(np.asarray(rows, dtype=np.int32)))
    return G.cpu().numpy(), A.cpu().numpy(), b.cpu().numpy(), ne.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. dyadic inputs: bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("rank", RANKS)
def test_dyadic_bit_for_bit(rank, implicit):
    ref = reference(rank, implicit, True)
    assert ref["exact"], "the yardstick's sums depend on the order: the inputs are not exact"
    G, A, b, ne = run_normal_equations(ref, implicit)
    assert G.tobytes() == ref["G"].tobytes()
    assert np.array_equal(ne, ref["ne"])
    assert ne[CASE_ROWS["nonpositive"]] == (0 if implicit else 6) and ne[CASE_ROWS["empty"]] == 0
    assert b.tobytes() == (ref["b"] + 0.0).tobytes()
    assert A.tobytes() == (ref["A"] + 0.0).tobytes()             # + 0.0: the device starts every sum from +0.0
    if implicit:
        assert not b[CASE_ROWS["nonpositive"]].any() and np.array_equal(A[CASE_ROWS["empty"]], ref["G"])


@pytest.mark.parametrize("rank", [10, 128])
@pytest.mark.parametrize("n", [4096, 4097, 2 * 4096 + 3])
def test_gram_blocks_bit_for_bit(rank, n):
    """more source rows than one block of the Gram sum: dyadic rows, so the float64 product is exact in any order"""
    F = make_factors(7, rank, True, n=n)
    G = eng().gram(dev(F)).cpu().numpy()
    assert G.tobytes() == (F.astype(np.float64).T @ F.astype(np.float64)).tobytes()
    assert np.array_equal(eng().gram(dev(F[:0])).cpu().numpy(), np.zeros((rank, rank)))


# ---------------------------------------------------------------------------------------------------------------------
# 2. general inputs: within (n + n_G + 2) 2^-53 sum |terms|
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("rank", RANKS)
def test_general_within_the_sum_bound(rank, implicit):
    ref = reference(rank, implicit, False)
    G, A, b, ne = run_normal_equations(ref, implicit)
    lens = np.diff(ref["side"][0])
    n_G = N_SRC if implicit else 0
    worst = 0.0
    tol_g = R.tolerance("sum", n=0, n_G=N_SRC, abs_terms=ref["Gs"])
    worst = max(worst, ratio(np.abs(G - ref["G"]), tol_g))
    assert (np.abs(G - ref["G"]) <= tol_g).all()
    assert np.array_equal(ne, ref["ne"])
    for row, n in enumerate(lens):
        tol_a = R.tolerance("sum", n=int(n), n_G=n_G, abs_terms=ref["SA"][row])
        tol_b = R.tolerance("sum", n=int(n), n_G=0, abs_terms=ref["Sb"][row])
        err_a, err_b = np.abs(A[row] - ref["A"][row]), np.abs(b[row] - ref["b"][row])
        assert (err_a <= tol_a).all() and (err_b <= tol_b).all(), row
        worst = max(worst, ratio(err_a, tol_a), ratio(err_b, tol_b))
    print(f"als sums rank={rank} implicit={implicit}: worst error / bound = {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the solve, 4. layout independence
# ---------------------------------------------------------------------------------------------------------------------
def run_half_step(ref, implicit, reg, rows=None, X=None):
    e = eng()
    F = dev(ref["F"])
    side = device_side(ref["side"])
    n_dst, r = side[0].numel() - 1, F.shape[1]
    X = torch.full((n_dst, r), 7.0, dtype=torch.float32, device="cuda") if X is None else X
    has = torch.full((n_dst,), 9, dtype=torch.uint8, device="cuda")
    failed = torch.zeros(1, dtype=torch.int32, device="cuda")
    e.half_step(side, F, e.gram(F) if implicit else None, implicit, ref["alpha"], reg, X, has, failed,
                rows=None if rows is None else dev(np.asarray(rows, dtype=np.int32)))
    return X.cpu().numpy(), has.cpu().numpy(), int(failed.item())


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("rank", RANKS)
def test_solve_within_the_cholesky_bound(rank, implicit):
    ref = reference(rank, implicit, False)
    reg = 0.1
    _, A, b, ne = run_normal_equations(ref, implicit)
    X, has, failed = run_half_step(ref, implicit, reg)
    lens = np.diff(ref["side"][0])
    assert np.array_equal(has[lens == 0], np.zeros((lens == 0).sum(), dtype=np.uint8)) and not X[lens == 0].any()
    worst, tested = 0.0, 0
    for row, n in enumerate(lens):
        if n == 0 or not (ne[row] >= 1 or N_SRC >= rank):
            continue                                             # the issue's condition on a tested row
        kappa = R.kappa2(A[row], reg, ne[row])
        assert kappa <= 1e6, (row, kappa)
        x = R.solve(A[row], b[row], reg, ne[row])
        tol = R.tolerance("solve", r=rank, kappa=kappa, x=x)
        err = np.abs(X[row].astype(np.float64) - x)
        assert has[row] == 1 and (err <= tol).all(), (row, ratio(err, tol))
        worst, tested = max(worst, ratio(err, tol)), tested + 1
    assert tested >= 18 and failed <= 1        # only the all-non-positive row over a rank-deficient G may fail to factorise
    print(f"als solve rank={rank} implicit={implicit}: worst error / bound = {worst:.4f} over {tested} rows")


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("rank", RANKS)
def test_layout_independence(rank, implicit):
    ref = dict(side=make_side(3, False), F=make_factors(100 + rank, rank, False), alpha=1.0)      # no yardstick needed
    n_dst = len(ref["side"][0]) - 1
    X0, has0, _ = run_half_step(ref, implicit, 0.1)
    X1, has1, _ = run_half_step(ref, implicit, 0.1)
    assert X0.tobytes() == X1.tobytes() and has0.tobytes() == has1.tobytes()
    Xr, hasr, _ = run_half_step(ref, implicit, 0.1, rows=list(range(n_dst))[::-1])
    assert Xr.tobytes() == X0.tobytes() and hasr.tobytes() == has0.tobytes()
    long_row = CASE_ROWS["split"]
    Xl, hasl, _ = run_half_step(ref, implicit, 0.1, rows=[long_row])
    assert Xl[long_row].tobytes() == X0[long_row].tobytes() and hasl[long_row] == 1
    untouched = np.arange(n_dst) != long_row
    assert (Xl[untouched] == 7.0).all() and (hasl[untouched] == 9).all()          # rows outside the list are not written
    assert np.isfinite(X0).all() and X0[long_row].any()


def test_unannounced_pieces_are_reported():
    """n_pieces sizes the workspace; a long row beyond it is not computed and counts as failed"""
    ref = dict(side=make_side(3, False), F=make_factors(110, 10, False), alpha=1.0)
    e = eng()
    F, side = dev(ref["F"]), device_side(ref["side"])
    X = torch.zeros((20, 10), dtype=torch.float32, device="cuda")
    has, failed = torch.zeros(20, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    e.half_step(side, F, e.gram(F), True, 1.0, 0.1, X, has, failed, n_pieces=2)       # P + 1 needs 2, 2P + 3 three more
    assert int(failed.item()) == 1 and has.cpu().numpy()[[5, 6]].tolist() == [1, 0]
    full, _, _ = run_half_step(ref, True, 0.1)
    assert X.cpu().numpy()[:6].tobytes() == full[:6].tobytes() and not X.cpu().numpy()[6].any()


def test_singular_system_raises_the_counter():
    """explicit mode, reg = 0, every source row the zero vector: A = 0, the first pivot is not positive"""
    e = eng()
    side = device_side((np.array([0, 2, 3]), np.array([0, 1, 1], dtype=np.int32), np.array([1.0, 2.0, 3.0])))
    F = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
    X = torch.ones((2, 4), dtype=torch.float32, device="cuda")
    has, failed = torch.ones(2, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    e.half_step(side, F, None, False, 1.0, 0.0, X, has, failed)
    assert int(failed.item()) == 2 and not X.cpu().numpy().any() and not has.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. top-k
# ---------------------------------------------------------------------------------------------------------------------
def topk_case(n_items, rank, seed=0):
    rng = np.random.default_rng(1000 * n_items + rank + seed)
    n_users = 14
    U = rng.normal(size=(n_users, rank)).astype(np.float32)
    V = rng.normal(size=(n_items, rank)).astype(np.float32)
    if n_items > 20:
        V[n_items // 2:] = V[np.arange(n_items - n_items // 2) % 7]                # many exactly equal scores
    has_u, has_v = np.ones(n_users, dtype=np.uint8), np.ones(n_items, dtype=np.uint8)
    has_u[3] = 0
    if n_items > 2:
        has_v[[2, n_items - 1]] = 0
    seen = [np.sort(rng.choice(n_items, rng.integers(0, n_items // 2 + 1), replace=False)) for _ in range(n_users)]
    seen[1] = np.arange(n_items)                                                   # has seen everything
    seen[2] = np.repeat(seen[2], 2)                                                # a log lists a pair twice
    off = np.zeros(n_users + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seen])
    queries = np.array(list(range(n_users)) + [n_users + 5, 0, -1], dtype=np.int32)
    return U, V, has_u, has_v, seen, off, queries


def check_topk(e, case, k, mask):
    U, V, has_u, has_v, seen, off, queries = case
    n_users, n_items, r = U.shape[0], V.shape[0], U.shape[1]
    dU, dV, dhu, dhv = dev(U), dev(V), dev(has_u), dev(has_v)
    seen_dev = (dev(off), dev(np.concatenate(seen).astype(np.int32)))
    ids, vals, cnt = e.topk(dev(queries), dU, dhu, dV, dhv, k, mask=None if mask is None else dev(mask), seen=seen_dev)
    ids, vals, cnt = ids.cpu().numpy(), vals.cpu().numpy(), cnt.cpu().numpy()
    # the device's own pair scores of every (user, item): the same function, so the list must be their exact order
    pu, pi = np.repeat(np.arange(n_users), n_items).astype(np.int32), np.tile(np.arange(n_items), n_users).astype(np.int32)
    ps, pv = e.pair_scores(dev(pu), dev(pi), dU, dhu, dV, dhv)
    ps, pv = ps.cpu().numpy().reshape(n_users, n_items), pv.cpu().numpy().reshape(n_users, n_items)
    assert np.array_equal(pv != 0, (has_u[:, None] != 0) & (has_v[None, :] != 0))
    dot, absdot = R.dots(U, V)
    worst = 0.0
    for q, u in enumerate(queries):
        if not (0 <= u < n_users) or not has_u[u]:
            assert cnt[q] == 0 and (ids[q] == -1).all() and np.isneginf(vals[q]).all()
            continue
        adm = has_v != 0
        if mask is not None:
            adm &= mask != 0
        adm[seen[u]] = False
        m = min(k, int(adm.sum()))
        assert cnt[q] == m and (ids[q, m:] == -1).all() and np.isneginf(vals[q, m:]).all()
        got, val = ids[q, :m], vals[q, :m]
        assert adm[got].all() and len(set(got.tolist())) == m
        tol = R.tolerance("score", r=r, abs_dot=absdot[u])
        err = np.abs(val.astype(np.float64) - dot[u, got])
        assert (err <= tol[got]).all()
        worst = max(worst, ratio(err, tol[got]))
        assert (val[:-1] >= val[1:]).all() and (got[:-1] < got[1:])[val[:-1] == val[1:]].all()     # ties by id ascending
        out = adm.copy()
        out[got] = False
        if m == k and out.any():
            assert (dot[u, out] <= float(val[-1]) + tol[out]).all()                                # the certificate
        assert val.tobytes() == ps[u, got].tobytes()                                               # one score function
        cand = np.nonzero(adm)[0]
        order = cand[np.lexsort((cand, -ps[u, cand].astype(np.float64)))][:m]
        assert np.array_equal(got, order)
    return worst


@pytest.mark.parametrize("k", [1, 10, 64, 512])
@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 700])
def test_topk_certificate(n_items, k):
    e = eng()
    case = topk_case(n_items, 10)
    worst = check_topk(e, case, k, None)
    mask = np.zeros(n_items, dtype=np.uint8)
    mask[np.random.default_rng(n_items).choice(n_items, min(n_items, 5), replace=False)] = 1       # leaves fewer than k
    worst = max(worst, check_topk(e, case, k, mask))
    print(f"als top-k n_items={n_items} k={k}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("rank", [1, 33, 128])
def test_topk_other_ranks(rank):
    worst = check_topk(eng(), topk_case(700, rank), 64, None)
    print(f"als top-k rank={rank}: worst error / bound = {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the model
# ---------------------------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS, COLD_USER, COLD_ITEM = 40, 30, 17, 11


def model_log():
    rng = np.random.default_rng(21)
    rows = [(u, i) for u in range(N_USERS) for i in range(N_ITEMS)
            if u != COLD_USER and i != COLD_ITEM and (rng.random() < 0.3 or i == (u * 7) % N_ITEMS and i != COLD_ITEM)]
    rows += [(0, 1), (0, 1), (39, 29)] + [(u, 0) for u in range(N_USERS) if u != COLD_USER]
    user, item = np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64)
    rel = rng.integers(1, 6, len(rows)).astype(np.float64)
    rel[::9] = 0.0
    rel[4::13] *= -1.0
    return pd.DataFrame({"user_idx": user, "item_idx": item, "relevance": rel})


@pytest.fixture(scope="module")
def fitted():
    from replay_cql_amd.als import ALSWrap
    log = model_log()
    m1, m2 = ALSWrap(rank=10, seed=7, max_iter=1), ALSWrap(rank=10, seed=7, max_iter=2)
    m1.fit(log)
    m2.fit(log)
    return log, m1, m2


def test_model_iterations_follow_the_yardstick(fitted):
    log, m1, m2 = fitted
    user, item, rel = (log[c].to_numpy() for c in ("user_idx", "item_idx", "relevance"))
    item_side, user_side = R.sides(user, item, rel, N_USERS, N_ITEMS)
    U0 = m1._init_factors(N_USERS, 10, 7).cpu().numpy()
    assert np.allclose(np.linalg.norm(U0.astype(np.float64), axis=1), 1.0, atol=1e-6)
    U1, V1 = (m1.factors_device(e)[0].cpu().numpy() for e in ("user", "item"))
    U2, V2 = (m2.factors_device(e)[0].cpu().numpy() for e in ("user", "item"))
    has_u, has_v = (m2.factors_device(e)[1].cpu().numpy() for e in ("user", "item"))
    assert has_u.sum() == N_USERS - 1 and not has_u[COLD_USER] and has_v.sum() == N_ITEMS - 1 and not has_v[COLD_ITEM]
    assert not U2[COLD_USER].any() and not V2[COLD_ITEM].any()
    worst = 0.0
    for side, F, X in ((item_side, U1, V2), (user_side, V2, U2)):
        G, Gs, _ = R.gram(F)
        A, b, ne = R.normal_equations(side, F, True, 1.0, G)[:3]
        for row in range(len(side[0]) - 1):
            if side[0][row + 1] == side[0][row]:
                continue
            kappa = R.kappa2(A[row], 0.1, ne[row])
            assert kappa <= 1e6
            x = R.solve(A[row], b[row], 0.1, ne[row])
            tol = R.tolerance("solve", r=10, kappa=kappa, x=x)
            err = np.abs(X[row].astype(np.float64) - x)
            assert (err <= tol).all(), (row, ratio(err, tol))
            worst = max(worst, ratio(err, tol))
    print(f"als model steps: worst error / bound = {worst:.4f}")


def test_model_predictions_agree(fitted, tmp_path):
    from replay_cql_amd.als import ALSWrap
    log, _, m = fitted
    k = 5
    recs = m.predict(log, k)
    assert list(recs.columns) == ["user_idx", "item_idx", "relevance"] and len(recs) == (N_USERS - 1) * k
    assert COLD_USER not in set(recs["user_idx"]) and COLD_ITEM not in set(recs["item_idx"])
    assert recs.merge(log[["user_idx", "item_idx"]].drop_duplicates(), on=["user_idx", "item_idx"]).empty     # nothing seen
    dlog = {c: torch.as_tensor(log[c].to_numpy()).cuda() for c in log.columns}
    rd = m.recommend(dlog, k)
    rd = pd.DataFrame({c: rd[c].cpu().numpy() for c in ("user_idx", "item_idx", "relevance")})
    assert rd.equals(recs.astype(rd.dtypes.to_dict()))
    pairs = m.predict_pairs(recs[["user_idx", "item_idx"]], log)
    assert pairs["relevance"].to_numpy().tobytes() == recs["relevance"].to_numpy().tobytes()
    cold = m.predict_pairs(pd.DataFrame({"user_idx": [COLD_USER, 0, 0, 99], "item_idx": [0, COLD_ITEM, 3, 0]}), log)
    assert cold[["user_idx", "item_idx"]].values.tolist() == [[0, 3]]
    # the factors handed to a reranker reproduce the scores
    uf, rank = m._get_features(pd.DataFrame({"user_idx": [0, COLD_USER, 5, 99]}), None)
    itf, _ = m._get_features(pd.DataFrame({"item_idx": np.arange(N_ITEMS)}), None)
    assert rank == 10 and list(uf.columns) == ["user_idx", "user_factors"] and list(itf.columns) == ["item_idx", "item_factors"]
    assert uf["user_factors"][1] is None and uf["user_factors"][3] is None and itf["item_factors"][COLD_ITEM] is None
    U, V = (m.factors_device(e)[0].cpu().numpy() for e in ("user", "item"))
    assert np.array_equal(np.array(uf["user_factors"][2], dtype=np.float32), U[5])
    vec = m._get_item_vectors()
    assert vec["item_idx"].tolist() == [i for i in range(N_ITEMS) if i != COLD_ITEM]
    assert np.array_equal(np.stack(vec["item_vector"].to_numpy()), V[vec["item_idx"].to_numpy()])
    dot, absdot = R.dots(U, V)
    ru, ri = recs["user_idx"].to_numpy(), recs["item_idx"].to_numpy()
    assert (np.abs(recs["relevance"].to_numpy() - dot[ru, ri]) <= R.tolerance("score", r=10, abs_dot=absdot[ru, ri])).all()
    # an item subset goes through the mask; seen items may come back when asked for
    sub = m.predict(log, 3, users=[0, 5], items=[1, 2, 3, 4, COLD_ITEM, 77], filter_seen_items=False)
    assert set(sub["item_idx"]) <= {1, 2, 3, 4} and sub.groupby("user_idx").size().tolist() == [3, 3]
    # save, load
    path = str(tmp_path / "als.pt")
    m._save_model(path)
    m2 = ALSWrap()
    m2._load_model(path)
    assert m2._init_args == m._init_args and m2.max_iter == 2
    assert m2.predict(log, k).equals(recs)


def test_model_fits_the_same_from_every_kind_of_log(fitted):
    import pyarrow as pa
    from replay_cql_amd.als import ALSWrap
    log, _, m = fitted
    arrow, ddict = ALSWrap(rank=10, seed=7, max_iter=2), ALSWrap(rank=10, seed=7, max_iter=2)
    arrow.fit(pa.Table.from_pandas(log))
    ddict.fit({c: torch.as_tensor(log[c].to_numpy()).cuda() for c in log.columns})
    for other in (arrow, ddict):
        for e in ("user", "item"):
            assert all(torch.equal(a, b) for a, b in zip(m.factors_device(e), other.factors_device(e)))
        assert other.fit_users["user_idx"].tolist() == sorted(m.fit_users["user_idx"].tolist())
    other_seed = ALSWrap(rank=10, seed=8, max_iter=2)
    other_seed.fit(log)
    assert not torch.equal(other_seed.factors_device("user")[0], m.factors_device("user")[0])


def test_model_errors():
    from replay_cql_amd.als import ALSWrap
    log = model_log()
    bad = log.copy()
    bad.loc[3, "relevance"] = np.nan
    with pytest.raises(ValueError, match="relevance contains NaN"):
        ALSWrap(max_iter=1).fit(bad)

    class ZeroStart(ALSWrap):
        def _init_factors(self, n, rank, seed, device=None):
            return torch.zeros_like(super()._init_factors(n, rank, seed, device))

    with pytest.raises(ValueError, match="not positive definite"):                 # a singular system, not a GPU fault
        ZeroStart(rank=4, implicit_prefs=False, max_iter=1, reg_param=0.0).fit(log)
    m = ALSWrap(rank=4, max_iter=1)
    m.fit(log)
    with pytest.raises(ValueError, match="k must be in 1..512"):
        m.recommend(log, 513)
