"""ADMM SLIM on the GPU (replay_cql_amd.admm_slim, section f11: csrc/dense.hip) against the yardstick
tests/admm_slim_reference.py and tests/golden/admm_slim_known_answers.json.

Every tolerance is derived, none is fitted (u = 2^-53, gamma_m = m u / (1 - m u), evaluated in longdouble):
  GEMM        dyadic data: the bytes of numpy; random data: gamma_{k+2} (|alpha| |A| |op(B)| + |beta| |E|) per element
  Gram        integer data: the bytes of numpy
  inverse     max |A X - I| <= 8 max(the same residual of numpy.linalg.inv, u): the floor of one rounding only keeps the
              bound from being 0 where numpy's 1 x 1 or 2 x 2 inverse happens to be exact
  iteration   DESIGN.md section 3.14: with A_T = |P| + |W| (rho |C| + |Gamma|),
              e_B = gamma_{n+7} (A_T_ij + |W_ij| A_T_jj / |W_jj|),  e_C = e_B + 4 u (|B| + |Gamma| / rho + c),
              e_Gamma = rho (e_B + e_C) + 4 u (rho (|B| + |C'|) + |Gamma|), against the longdouble iteration on the same
              fp64 state; a norm |x| within |e_x|_F + gamma_{n^2+2} |x|
  whole fit   the same iteration count and rho sequence; C within 32 x the case's own float64-vs-longdouble spread
              (tests/golden, recomputed by the CPU test), floor 2^-48 max |C|"""
import json
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import admm_slim_reference as AR
import neighbour_reference as NR
from replay_cql_amd import _native as N
from replay_cql_amd._dense import Dense
from replay_cql_amd.admm_slim import ADMMSLIM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "admm_slim_known_answers.json").read_text())
LD = np.longdouble
U = LD(2) ** -53
_CACHE = {}


def gamma(m):
    return LD(m) * U / (1 - LD(m) * U)


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def eng():
    return cached("engine", lambda: Dense(torch.device(DEV)))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def padded(a, extra=3):
    """a device tensor equal to `a` whose rows lie `extra` elements apart from being contiguous"""
    buf = torch.full((a.shape[0], a.shape[1] + extra), 7.5, dtype=torch.float64, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


# ------------------------------------------------------------------------------------------------- GEMM
SHAPES = [(1, 1, 1), (16, 16, 4), (17, 15, 5), (64, 64, 64), (65, 130, 67), (257, 129, 255)]


def gemm_case(m, n, k, ta, tb, dyadic, seed=0):
    rs = np.random.RandomState(1000 * m + 10 * n + k + seed)
    draw = (lambda *s: rs.randint(-8, 9, size=s) / 8.0) if dyadic else (lambda *s: rs.standard_normal(s))
    A, B, E = draw(m, k), draw(k, n), draw(m, n)
    return A, B, E, (A.T.copy() if ta else A), (B.T.copy() if tb else B)


def run_gemm(As, Bs, E, alpha, beta, ta, tb):
    out = padded(np.zeros(E.shape))
    eng().gemm(padded(As), padded(Bs), padded(E) if beta != 0 else None, alpha, beta, ta, tb, out=out)
    return out.cpu().numpy()


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-0.5, 2.0)])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_dyadic_equals_numpy_bit_for_bit(m, n, k, alpha, beta, ta, tb):
    A, B, E, As, Bs = gemm_case(m, n, k, ta, tb, dyadic=True)
    ref = alpha * (A @ B)
    if beta != 0:
        ref = ref + beta * E
    got = run_gemm(As, Bs, E, alpha, beta, ta, tb)
    assert got.tobytes() == ref.tobytes(), np.argwhere(got != ref)[:5].tolist()
    assert run_gemm(As, Bs, E, alpha, beta, ta, tb).tobytes() == got.tobytes()


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-0.5, 2.0)])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_random_within_the_derived_bound(m, n, k, alpha, beta, ta, tb):
    A, B, E, As, Bs = gemm_case(m, n, k, ta, tb, dyadic=False)
    got = run_gemm(As, Bs, E, alpha, beta, ta, tb)
    ref = LD(alpha) * (A.astype(LD) @ B.astype(LD)) + LD(beta) * E.astype(LD)
    bound = gamma(k + 2) * (abs(LD(alpha)) * (np.abs(A).astype(LD) @ np.abs(B).astype(LD)) + abs(LD(beta)) * np.abs(E).astype(LD))
    err = np.abs(got.astype(LD) - ref)
    print(f"gemm {m}x{n}x{k} ta={ta} tb={tb} a={alpha} b={beta}: worst error / bound = {float(np.max(err / bound)):.3g}")
    assert (err <= bound).all()
    assert run_gemm(As, Bs, E, alpha, beta, ta, tb).tobytes() == got.tobytes()


def test_gemm_rejects_bad_arguments_without_a_launch():
    a = dev(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="shapes"):
        eng().gemm(a, dev(np.zeros((3, 4))))
    with pytest.raises(N.CqlrecError, match="leading dimension"):
        eng().call("dense_gemm_f64", a, 3, 0, a, 4, 0, None, 0, 1.0, 0.0, 4, 4, 4, a, 4)


# ------------------------------------------------------------------------------------------------- Gram
def views(user, item, rel, n_users, n_items):
    D = eng()
    u, i, r = dev(user.astype(np.int32)), dev(item.astype(np.int32)), dev(rel.astype(np.float64))
    perm_i, off_i = D.segments(i, n_items, u.to(torch.int64))
    perm_u, off_u = D.segments(u, n_users, i.to(torch.int64))
    perm_i, perm_u = perm_i.long(), perm_u.long()
    return ((off_i, u[perm_i].contiguous(), r[perm_i].contiguous()), (off_u, i[perm_u].contiguous(), r[perm_u].contiguous()))


def test_gram_equals_numpy_bit_for_bit_with_duplicates_empty_items_and_a_cut_row():
    piece = N.DENSE_GRAM_PIECE
    assert piece == 1024
    rs = np.random.RandomState(7)
    n_users, n_items = 2 * piece + 300, 37
    present = rs.rand(n_users, n_items) < 0.08
    present[:, 5] = True                                  # a row of 2 pieces and a rest
    present[:, [0, 11, 36]] = False                       # items without rows, the first and the last among them
    user, item = np.nonzero(present)
    dup = rs.choice(len(user), size=len(user) // 5, replace=False)
    at_cut = np.nonzero((item == 5) & np.isin(user, [piece - 1, piece, 2 * piece - 1]))[0]   # runs across the cuts of row 5
    user = np.concatenate([user, user[dup], user[at_cut], user[at_cut]])
    item = np.concatenate([item, item[dup], item[at_cut], item[at_cut]])
    order = rs.permutation(len(user))
    user, item = user[order], item[order]
    rel = rs.randint(1, 6, size=len(user)).astype(np.float64)
    X = AR.interactions(user, item, rel, n_users, n_items)
    ref = X.T @ X
    got = eng().gram(*views(user, item, rel, n_users, n_items), n_items, n_users).cpu().numpy()
    assert got.tobytes() == ref.tobytes(), np.argwhere(got != ref)[:5].tolist()
    assert (got[[0, 11, 36]] == 0).all() and got[5, 5] > piece
    case = GOLDEN["gram_duplicates"]
    u, i, r = (np.array(case[c]) for c in ("user", "item", "relevance"))
    small = eng().gram(*views(u, i, r.astype(np.float64), 2, 2), 2, 2).cpu().numpy()
    assert small.tolist() == case["G"]


# ------------------------------------------------------------------------------------------------- the inverse
def spd_matrix(n, seed=3):
    rs = np.random.RandomState(seed + n)
    X = (rs.rand(3 * n + 5, n) < 0.2).astype(np.float64)
    return X.T @ X + 8.0 * np.eye(n)


def residual(A, X):
    return float(np.max(np.abs(A.astype(LD) @ X.astype(LD) - np.eye(len(A), dtype=LD))))


@pytest.mark.parametrize("n", [1, 2, 17, 64, 65, 130, 257])
def test_inverse_residual_against_numpy(n):
    A = spd_matrix(n)
    got = eng().spd_inverse(padded(A)).cpu().numpy()
    shifted = eng().spd_inverse(dev(A - 8.0 * np.eye(n)), 8.0).cpu().numpy()
    assert shifted.tobytes() == got.tobytes() and (got == got.T).all()
    mine, theirs = residual(A, got), residual(A, np.linalg.inv(A))
    floor = float(U)
    print(f"inverse n={n}: residual {mine:.3g}, numpy.linalg.inv {theirs:.3g}, ratio to max(numpy, u) {mine / max(theirs, floor):.3g}")
    assert mine <= 8 * max(theirs, floor)


def test_inverse_known_answer_and_status_on_a_pivot_that_is_not_positive():
    case = GOLDEN["inverse_2x2"]
    got = eng().spd_inverse(dev(np.array(case["A"], dtype=np.float64))).cpu().numpy()
    assert np.allclose(3 * got, case["times_3"], rtol=0, atol=8 * float(U))
    with pytest.raises(ValueError, match="not positive definite: pivot 0 "):
        eng().spd_inverse(dev(-np.eye(3)))
    A = np.eye(70)
    A[65, 65] = 0.0
    with pytest.raises(ValueError, match="pivot 65 "):
        eng().spd_inverse(dev(A))
    with pytest.raises(ValueError, match="pivot 1 "):
        eng().spd_inverse(dev(np.ones((2, 2))))
    torch.cuda.synchronize()
    assert eng().spd_inverse(dev(np.eye(70))).cpu().numpy().tolist() == np.eye(70).tolist()   # the device is fine afterwards


# ------------------------------------------------------------------------------------------------- one iteration
def yardstick(index):
    return cached(("fit", index), lambda: AR.case_fit(AR.CASES[index], keep_states=(0, 3)))


def run_iteration(W, P, C, Gamma, rho, lambda_1):
    D = eng()
    n = len(W)
    c, g = dev(C), dev(Gamma)
    ws, sums = D._ws(D.ws_bytes("admm_iteration", n)), D._empty(5, torch.float64)
    D.admm_iteration(dev(W), dev(P), c, g, rho, lambda_1, ws, sums)
    return c.cpu().numpy(), g.cpu().numpy(), sums.cpu().numpy()


def iteration_bounds(W, P, C, Gamma, rho, lambda_1, B, C1):
    n = len(W)
    aW, r = np.abs(W).astype(LD), LD(rho)
    A_T = np.abs(P).astype(LD) + aW @ (r * np.abs(C).astype(LD) + np.abs(Gamma).astype(LD))
    e_B = gamma(n + 7) * (A_T + aW * (np.diag(A_T) / np.abs(np.diag(W)).astype(LD))[None, :])
    e_C = e_B + 4 * U * (np.abs(B) + np.abs(Gamma).astype(LD) / r + LD(lambda_1) / r)
    e_G = r * (e_B + e_C) + 4 * U * (r * (np.abs(B) + np.abs(C1)) + np.abs(Gamma).astype(LD))
    return e_B, e_C, e_G


@pytest.mark.parametrize("index,it", [(0, 0), (0, 3), (3, 0), (3, 3)])
def test_one_iteration_from_the_yardsticks_state(index, it):
    lambda_1 = AR.CASES[index][3]
    W, P, C, Gamma, rho = yardstick(index)[1]["states"][it]
    n = len(W)
    B, C1, G1, norms = AR.iteration(*(x.astype(LD) for x in (W, P, C, Gamma)), LD(rho), LD(lambda_1))
    e_B, e_C, e_G = iteration_bounds(W, P, C, Gamma, rho, lambda_1, B, C1)
    got_C, got_G, sums = run_iteration(W, P, C, Gamma, rho, lambda_1)
    err_C, err_G = np.abs(got_C.astype(LD) - C1), np.abs(got_G.astype(LD) - G1)
    print(f"iteration case {index} it {it}: worst error / bound C' {float(np.max(err_C / e_C)):.3g}, Gamma' {float(np.max(err_G / e_G)):.3g}")
    assert (err_C <= e_C).all() and (err_G <= e_G).all()
    flipped = (got_C != 0) != (C1 != 0)
    assert (np.abs(got_C[flipped]) <= e_C[flipped]).all() and (np.abs(C1[flipped]) <= e_C[flipped]).all()
    fro = lambda x: np.sqrt(np.sum(x * x))            # noqa: E731
    e_norm = [fro(e_B + e_C), fro(e_C), fro(e_B), fro(e_C), fro(e_G)]
    for q in range(5):
        assert abs(np.sqrt(LD(sums[q])) - norms[q]) <= e_norm[q] + gamma(n * n + 2) * norms[q], q
    again = run_iteration(W, P, C, Gamma, rho, lambda_1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (got_C, got_G, sums)))


def test_one_iteration_known_answers():
    for name in ("iteration_2x2", "iteration_3x3"):
        case = GOLDEN[name]
        arrays = [np.array(case[k], dtype=np.float64) for k in ("W", "P", "C", "Gamma")]
        got_C, got_G, sums = run_iteration(*arrays, case["rho"], case["lambda_1"])
        assert got_C.tolist() == case["C1"] and got_G.tolist() == case["Gamma1"], name      # dyadic: exact
        assert sums.tolist() == case["squares"], name


# ------------------------------------------------------------------------------------------------- whole fits
def frame(user, item, rel):
    return pd.DataFrame({"user_idx": user.astype(np.int64), "item_idx": item.astype(np.int64), "relevance": rel})


def as_arrow(df):
    import pyarrow as pa
    return pa.Table.from_pandas(df, preserve_index=False)


def as_device(df):
    return {c: torch.as_tensor(df[c].to_numpy()).to(DEV) for c in df.columns}


def dense(model, n=None):
    off, col, val = (x.cpu().numpy() for x in model.similarity_device)
    n = len(off) - 1 if n is None else n
    C = np.zeros((n, n))
    C[np.repeat(np.arange(len(off) - 1), np.diff(off)), col] = val
    return C


def fitted(index, **attrs):
    def make():
        (user, item, rel), _ = yardstick(index)
        _, _, _, lam1, lam2, seed, _ = AR.CASES[index]
        model = ADMMSLIM(lam1, lam2, seed)
        for k, v in attrs.items():
            setattr(model, k, v)
        model.fit(frame(user, item, rel))
        return model
    return cached(("model", index, tuple(sorted(attrs.items()))), make)


@pytest.mark.parametrize("index", range(len(AR.CASES)))
def test_whole_fit_against_the_yardstick(index):
    _, ref = yardstick(index)
    stored = GOLDEN["whole_fit"][index]
    assert stored["case"] == list(AR.CASES[index])
    assert ref["branch_margin"] >= 1e-6 and ref["stop_margin"] >= 1e-6      # a flipped branch is never rounding
    model = fitted(index)
    assert model.n_iterations == ref["iterations"] == stored["iterations"]
    assert model.rho_sequence == ref["rho"] == stored["rho"] and model.rho == ref["rho"][-1]
    C = dense(model)
    tol = max(32 * stored["spread"], 2.0 ** -48 * float(np.max(np.abs(ref["C"]))))
    err = np.abs(C - ref["C"])
    print(f"whole fit case {index}: max |C - C_ref| = {err.max():.3g}, tolerance {tol:.3g}, "
          f"pattern differences {int(((C != 0) != (ref['C'] != 0)).sum())}")
    assert err.max() <= tol
    flipped = (C != 0) != (ref["C"] != 0)
    assert (np.abs(C[flipped]) <= tol).all() and (np.abs(ref["C"][flipped]) <= tol).all()
    assert np.allclose(model.residuals, ref["residuals"], rtol=1e-9, atol=0)


def test_max_iteration_one_and_lambda_1_zero():
    (user, item, rel), _ = yardstick(0)
    n_users, n_items, _, lam1, lam2, seed, _ = AR.CASES[0]
    X = AR.interactions(user, item, rel, n_users, n_items)
    model = fitted(0, max_iteration=1)
    ref = AR.fit(X, lam1, lam2, seed, max_iteration=1)
    assert model.n_iterations == 1 and model.rho_sequence == ref["rho"]
    tol = 2.0 ** -48 * float(np.max(np.abs(ref["C"])))
    assert np.abs(dense(model) - ref["C"]).max() <= tol
    # lambda_1 = 0 thresholds nothing: one iteration keeps all n^2 entries.  A whole fit keeps every entry off the
    # diagonal; ON it the constraint diag(B) = 0 drives C_jj = B_jj + Gamma_jj / rho to zero (Gamma_jj' = Gamma_jj -
    # Gamma_jj from the second iteration on), in the yardstick too, in float64 and in longdouble: zero or rounding noise
    model = ADMMSLIM(0, lam2, seed)
    model.max_iteration = 1
    model.fit(frame(user, item, rel))
    assert model.similarity_device[1].numel() == n_items * n_items == len(model.similarity)
    model = ADMMSLIM(0, lam2, seed)
    model.fit(frame(user, item, rel))
    C, ref = dense(model), AR.fit(X, 0, lam2, seed)
    assert model.n_iterations == ref["iterations"] > 1 and model.rho_sequence == ref["rho"]
    off_diagonal = ~np.eye(n_items, dtype=bool)
    assert (C[off_diagonal] != 0).all() and (ref["C"][off_diagonal] != 0).all()
    assert np.abs(np.diag(C)).max() <= 2.0 ** -48 * float(np.max(np.abs(ref["C"])))


def test_the_same_bytes_from_every_kind_of_log_and_from_two_fits_in_a_row():
    (user, item, rel), _ = yardstick(1)
    df = frame(user, item, rel)
    first = fitted(1)
    want = [x.cpu().numpy().tobytes() for x in first.similarity_device]
    for log in (as_arrow(df), as_device(df)):
        other = ADMMSLIM(*AR.CASES[1][3:6])
        other.fit(log)
        assert [x.cpu().numpy().tobytes() for x in other.similarity_device] == want
    first.fit(df)                                          # starts from rho = lambda_2 again, not from the last rho
    assert [x.cpu().numpy().tobytes() for x in first.similarity_device] == want


def test_similarity_frame_order_and_dtypes():
    model = fitted(1)
    sim = model.similarity
    assert list(sim.columns) == ["item_idx_one", "item_idx_two", "similarity"]
    assert [str(t) for t in sim.dtypes] == ["int32", "int32", "float64"]
    C = dense(model)
    rows, cols = np.nonzero(C)                             # row-major
    assert sim["item_idx_one"].tolist() == rows.tolist() and sim["item_idx_two"].tolist() == cols.tolist()
    assert sim["similarity"].tolist() == C[rows, cols].tolist() and (sim["similarity"] != 0).all()
    off, col, val = model.similarity_device
    assert off.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float64
    assert model._dataframes["similarity"] is sim
    near = model.get_nearest_items([3, 5], k=4)
    assert list(near.columns) == ["item_idx", "neighbour_item_idx", "similarity"]
    for i in (3, 5):
        best = sorted(zip(-C[i][C[i] != 0], np.nonzero(C[i])[0]))[:4]
        assert sorted(near[near["item_idx"] == i]["neighbour_item_idx"]) == sorted(int(j) for _, j in best)


def close_lists(got, ref, scale):
    """[(j, score)] equal up to the rounding of a sum: scores within tol, ids equal except across a tie within tol"""
    tol = 64 * float(U) * scale
    assert len(got) == len(ref)
    ref_score = dict(ref)
    for (gj, gs), (rj, rs) in zip(got, ref):
        assert abs(gs - rs) <= tol
        assert gj == rj or abs(ref_score[gj] - rs) <= tol


@pytest.mark.parametrize("filter_seen", [True, False])
def test_predictions_equal_the_dense_product_under_the_tie_rule(filter_seen):
    (user, item, rel), _ = yardstick(1)
    n_users, n_items = AR.CASES[1][:2]
    model = fitted(1)
    C = dense(model)
    sim = {i: [(int(j), float(C[i, j])) for j in np.nonzero(C[i])[0]] for i in range(n_items)}
    rs = np.random.RandomState(5)
    log_user = np.concatenate([user, user[:40]])           # duplicated rows count twice
    log_item = np.concatenate([item, item[:40]])
    log = frame(log_user, log_item, np.ones(len(log_user)))
    scale = float(np.abs(C).max()) * 64
    for users, items in ((None, None), (rs.permutation(n_users)[:25], rs.permutation(n_items)[:30])):
        us = np.unique(log_user) if users is None else users
        its = np.arange(n_items) if items is None else items
        ref = NR.predict(sim, log_user, log_item, us, its, 7, filter_seen)
        out = model.recommend(log, 7, users, items, filter_seen)
        got = {}
        for u, j, s in zip(*(out[c].cpu().numpy() for c in ("user_idx", "item_idx", "relevance"))):
            got.setdefault(int(u), []).append((int(j), float(s)))
        cnt = np.zeros((n_users, n_items))
        np.add.at(cnt, (log_user, log_item), 1.0)
        for u in us:
            close_lists(got.get(int(u), []), ref[int(u)], scale)
            full = cnt[int(u)] @ C                         # the dense product: the score of every listed item
            for j, s in got.get(int(u), []):
                assert abs(full[j] - s) <= 64 * float(U) * scale
        frame_out = model.predict(log, 7, users=None if users is None else list(users), items=None if items is None else list(items),
                                  filter_seen_items=filter_seen)
        assert len(frame_out) == sum(len(v) for v in got.values())
    pairs = pd.DataFrame({"user_idx": rs.randint(0, n_users, 60), "item_idx": rs.randint(0, n_items, 60)}).drop_duplicates()
    ref = NR.pair_scores(sim, log_user, log_item, list(zip(pairs["user_idx"], pairs["item_idx"])))
    out = model.predict_pairs(pairs, log)
    got = {(int(u), int(j)): float(s) for u, j, s in zip(out["user_idx"], out["item_idx"], out["relevance"])}
    for (u, j), r in zip(zip(pairs["user_idx"], pairs["item_idx"]), ref):
        if r is None:
            assert (int(u), int(j)) not in got
        else:
            assert abs(got[(int(u), int(j))] - r) <= 64 * float(U) * scale


def test_the_other_neighbourhood_models_keep_their_bytes_beside_an_admm_slim_fit():
    from replay_cql_amd.association_rules import AssociationRulesItemRec
    from replay_cql_amd.neighbour import ItemKNN
    (user, item, rel), _ = yardstick(2)
    df = frame(user, item, rel)

    def tables():
        knn, rules = ItemKNN(10), AssociationRulesItemRec(min_item_count=1, min_pair_count=1)
        knn.fit(df)
        rules.fit(df)
        return [x.cpu().numpy().tobytes() for m in (knn, rules) for x in m.similarity_device]
    before = tables()
    model = ADMMSLIM(*AR.CASES[2][3:6])
    model.max_iteration = 2
    model.fit(df)
    assert tables() == before
