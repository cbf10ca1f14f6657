"""SLIM on the GPU (replay_cql_amd.slim, section f12: csrc/slim.hip) against the yardstick tests/slim_reference.py and
the recorded sklearn solutions of tests/golden/slim_known_answers.json.

What is pinned is the MINIMISER, by a certificate, not an iterate.  Every bound is derived in slim_reference.py:
  certificate   per column and coordinate |v_i| <= tol lambda_ + r_i: v the longdouble certificate of the device's w from
                the exact G, r the rounding of the device's float64 refresh and certificate; kkt[j] within max r of it
  beta > 0      |w - w'|_2 <= (|v|_2 + |v'|_2) / beta                      (strong convexity)
  beta = 0      F(w) - F(w') <= (|v|_inf + |v'|_inf) |w - w'|_1 + the rounding of the two evaluations of F
The shapes are the smallest that can go wrong: one and two items, around the wave of 64, more than one wave, and 1025
items, one more than the 1024 coordinates a workgroup screens at once; 4100 items, where a lane owns more than four
elements of a row and the kernel's loads run four deep with a rest (there the host checks a sample of the columns)."""
import json
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import neighbour_reference as NR
import slim_reference as SR
from replay_cql_amd import _native as N
from replay_cql_amd._dense import Dense
from replay_cql_amd.admm_slim import ADMMSLIM
from replay_cql_amd.slim import SLIM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "slim_known_answers.json").read_text())
LD = np.longdouble
_CACHE = {}

# n_items -> (n_users, p, seed, R)
SHAPES = {1: (6, 1.0, 11, 1), 2: (9, .6, 12, 1), 17: (60, .25, 13, 1), 63: (200, .12, 14, 5), 64: (200, .12, 15, 1),
          65: (200, .12, 16, 5), 130: (400, .08, 17, 1), 1025: (3000, .08, 18, 1), 4100: (2000, .08, 19, 1)}
SAMPLED = 4100                                              # certificates and distances on a sample of its columns



def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def frame(user, item, rel):
    return pd.DataFrame({"user_idx": user.astype(np.int64), "item_idx": item.astype(np.int64), "relevance": rel})


def as_arrow(df):
    import pyarrow as pa
    return pa.Table.from_pandas(df, preserve_index=False)


def as_device(df):
    return {c: torch.as_tensor(df[c].to_numpy()).to(DEV) for c in df.columns}


def shape_log(n):
    def make():
        n_users, p, seed, R = SHAPES[n]
        user, item, rel = SR.random_log(n_users, n, p, seed, R)
        X = SR.interactions(user, item, rel, n_users, n)
        return (user, item, rel), SR.exact_gram(X), n_users
    return cached(("log", n), make)


def golden_log(name):
    def make():
        spec = SR.GOLDEN_LOGS[name]
        c = GOLDEN["cases"][name]
        user, item, rel = (np.array(c[k]) for k in ("user", "item", "relevance"))
        return (user, item, rel.astype(np.float64)), SR.exact_gram(SR.interactions(user, item, rel, spec[0], spec[1])), spec[0]
    return cached(("golden", name), make)


def fit(rows, beta, lambda_, tol=None, max_iter=None, kind=frame):
    model = SLIM(beta, lambda_)
    if tol is not None:
        model.tol = tol
    if max_iter is not None:
        model.max_iter = max_iter
    log = frame(*rows)
    model.fit(log if kind is frame else kind(log))
    return model


def fitted(key, rows, beta, lambda_, tol):
    return cached(("model", key, beta, lambda_, tol), lambda: fit(rows, beta, lambda_, tol))


def dense(model, n):
    off, col, val = (x.cpu().numpy() for x in model.similarity_device)
    assert len(off) == n + 1
    S = np.zeros((n, n))
    S[np.repeat(np.arange(n), np.diff(off)), col] = val
    return S


def table_bytes(model):
    return [x.cpu().numpy().tobytes() for x in model.similarity_device] + [model.n_sweeps.cpu().numpy().tobytes(),
                                                                          model.kkt.cpu().numpy().tobytes()]


def check_certificate(model, G, nu, beta, lambda_, tol, label, columns=None):
    n = len(G)
    S, kkt, sweeps = dense(model, n), model.kkt.cpu().numpy(), model.n_sweeps.cpu().numpy()
    assert (S >= 0).all() and (np.diag(S) == 0).all()
    assert kkt.shape == (n,) and sweeps.shape == (n,) and sweeps.dtype == np.int32
    worst = worst_ratio = 0.0
    for j in range(n) if columns is None else columns:
        w = S[:, j]
        v, r = SR.certificate(G, j, w, nu, beta, lambda_), SR.refresh_rounding(G, j, w, nu, beta, lambda_)
        limit = LD(tol) * LD(lambda_) + r
        assert (np.abs(v) <= limit).all(), (label, j, float(np.max(np.abs(v) - limit)))
        assert abs(LD(kkt[j]) - np.max(np.abs(v))) <= np.max(r), (label, j)
        worst, worst_ratio = max(worst, float(np.max(np.abs(v)))), max(worst_ratio, float(np.max(np.abs(v) / limit)))
        assert sweeps[j] >= 1 if G[j, j] != 0 else (sweeps[j] == 0 and not w.any())
    assert model.n_not_converged == 0
    print(f"{label}: worst |v| {worst:.3g} (limit {tol * lambda_:.3g}), worst |v| / limit {worst_ratio:.3g}, sweeps median "
          f"{int(np.median(sweeps))} max {int(sweeps.max())}, updates {model.n_updates}, non-zeros {int((S != 0).sum())}")
    return S


# ------------------------------------------------------------------------------------------------- the certificate
@pytest.mark.parametrize("tol", [1e-9, 1e-4])
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_certificate_of_every_column(n, tol):
    rows, G, nu = shape_log(n)
    model = fitted(n, rows, 0.01, 0.01, tol)
    S = check_certificate(model, G, nu, 0.01, 0.01, tol, f"n={n} tol={tol:g}", columns_of(n) if n == SAMPLED else None)
    if n in (17, 65):                                        # not asserted: the float64 yardstick runs the same operations
        ref = SR.fit(G, nu, 0.01, 0.01, tol=tol)[0]
        print(f"n={n} tol={tol:g}: columns whose bytes equal the float64 yardstick's: {sum(S[:, j].tobytes() == ref[:, j].tobytes() for j in range(n))} of {n}")


@pytest.mark.parametrize("beta,lambda_", [(0.5, 0.001), (0, 0.01), (1e-3, 0.2)])
@pytest.mark.parametrize("tol", [1e-9, 1e-4])
def test_certificate_at_the_other_parameters(beta, lambda_, tol):
    rows, G, nu = shape_log(65)
    check_certificate(fitted(65, rows, beta, lambda_, tol), G, nu, beta, lambda_, tol, f"n=65 beta={beta} lambda_={lambda_} tol={tol:g}")


def test_negative_and_fractional_relevances_still_pass_the_certificate():
    n_users, n = 150, 40
    user, item, _ = SR.random_log(n_users, n, .15, 21, 1, duplicates=0.1)
    rel = np.random.RandomState(22).choice([-1.0, -0.5, 0.25, 0.5, 1.0, 1.5, 2.0], size=len(user))
    G = SR.exact_gram(SR.interactions(user, item, rel, n_users, n))
    for tol in (1e-9, 1e-4):
        model = fit((user, item, rel), 0.01, 0.01, tol)
        check_certificate(model, G, n_users, 0.01, 0.01, tol, f"signed fractional relevances tol={tol:g}")


# ------------------------------------------------------------------------------------------------- the minimiser
def columns_of(n):
    if n <= 130:
        return range(n)
    edges = {0, 1, 63, 64, 511, 1022, 1023, 1024, 3071, 3072, 4095, 4096, n - 1}
    return sorted({j for j in edges if j < n} | set(range(5, n, 97 if n <= 1025 else 211)))


@pytest.mark.parametrize("tol", [1e-9, 1e-4])
@pytest.mark.parametrize("n", [2, 17, 65, 130, 1025, 4100])
def test_distance_to_the_longdouble_minimiser(n, tol):
    beta, lambda_ = 0.01, 0.01
    rows, G, nu = shape_log(n)
    S = dense(fitted(n, rows, beta, lambda_, tol), n)
    worst = worst_ratio = 0.0
    for j in columns_of(n):
        ref = cached(("yardstick", n, j), lambda: SR.descend(G, j, nu, beta, lambda_, tol=1e-9, dtype=LD)[0])
        dist, bound = SR.distance_and_bound(G, j, S[:, j], ref, nu, beta, lambda_)
        assert dist <= bound, (j, float(dist), float(bound))
        worst, worst_ratio = max(worst, float(dist)), max(worst_ratio, float(dist / bound) if bound > 0 else 0.0)
    print(f"n={n} tol={tol:g}: worst |w - w_ref|_2 {worst:.3g}, worst ratio to the bound {worst_ratio:.3g}")


@pytest.mark.parametrize("tol", [1e-9, 1e-4])
@pytest.mark.parametrize("n", [17, 65])
def test_beta_zero_objective_gap(n, tol):
    beta, lambda_ = 0, 0.01
    rows, G, nu = shape_log(n)
    model = fitted(n, rows, beta, lambda_, tol)
    S = check_certificate(model, G, nu, beta, lambda_, tol, f"n={n} beta=0 tol={tol:g}")
    worst = -1.0
    for j in range(n):
        ref = cached(("yardstick0", n, j), lambda: SR.descend(G, j, nu, beta, lambda_, tol=1e-9, dtype=LD)[0])
        gap, bound = SR.objective_gap_and_bound(G, j, S[:, j], ref, nu, beta, lambda_)
        assert gap <= bound, (j, float(gap), float(bound))
        worst = max(worst, float(gap))
    print(f"n={n} beta=0 tol={tol:g}: worst F(w) - F(w_ref) {worst:.3g}")


@pytest.mark.parametrize("index", range(len(SR.GOLDEN_PARAMS)))
@pytest.mark.parametrize("name", sorted(SR.GOLDEN_LOGS))
def test_against_the_recorded_sklearn_solutions(name, index):
    beta, lambda_ = SR.GOLDEN_PARAMS[index]
    rows, G, nu = golden_log(name)
    rec = GOLDEN["cases"][name]["fits"][index]
    assert (rec["beta"], rec["lambda_"]) == (beta, lambda_)
    tight, default = np.array(rec["tight"]), np.array(rec["default"])
    n = len(G)
    model = fitted(name, rows, beta, lambda_, 1e-9)
    S = check_certificate(model, G, nu, beta, lambda_, 1e-9, f"{name} beta={beta} lambda_={lambda_}")
    worst = [0.0, 0.0]
    for j in range(n):
        if beta > 0:
            dist, bound = SR.distance_and_bound(G, j, S[:, j], tight[:, j], nu, beta, lambda_)
            assert dist <= bound, (j, float(dist), float(bound))
            far = np.sqrt(np.sum((S[:, j].astype(LD) - default[:, j]) ** 2))
            assert far <= LD(rec["spread_l2"]) + bound, (j, float(far))
            worst = [max(worst[0], float(dist)), max(worst[1], float(far))]
        else:
            for a, b in ((S[:, j], tight[:, j]), (tight[:, j], S[:, j]), (S[:, j], default[:, j])):
                gap, bound = SR.objective_gap_and_bound(G, j, a, b, nu, beta, lambda_)
                assert gap <= bound, (j, float(gap), float(bound))
    print(f"{name} beta={beta} lambda_={lambda_}: to sklearn tight {worst[0]:.3g}, to sklearn at the reference's settings {worst[1]:.3g} "
          f"(recorded spread {rec['spread_l2']:.3g})")
    if name == "duplicates":                                 # item 7 has no interactions: no row, and in no row
        sim = model.similarity
        assert 7 not in set(sim["item_idx_one"]) and 7 not in set(sim["item_idx_two"]) and len(sim) > 0
        assert int(model.n_sweeps[7]) == 0 and float(model.kkt[7]) == 0.0


# ------------------------------------------------------------------------------------------------- structure
def gram_on_device(rows, n_users, n_items):
    D = Dense(torch.device(DEV))
    user, item, rel = rows
    u, i, r = (torch.as_tensor(np.ascontiguousarray(a)).to(DEV) for a in (user.astype(np.int32), item.astype(np.int32), rel.astype(np.float64)))
    perm_i, off_i = D.segments(i, n_items, u.to(torch.int64))
    perm_u, off_u = D.segments(u, n_users, i.to(torch.int64))
    perm_i, perm_u = perm_i.long(), perm_u.long()
    return D, D.gram((off_i, u[perm_i].contiguous(), r[perm_i].contiguous()), (off_u, i[perm_u].contiguous(), r[perm_u].contiguous()),
                     n_items, n_users)


@pytest.mark.parametrize("n,ranges", [(130, [(0, 1), (129, 130), (60, 70), (3, 127)]), (1025, [(1020, 1025), (500, 530)])])
def test_a_column_range_gives_the_bytes_of_the_whole_fit(n, ranges):
    rows, G, nu = shape_log(n)
    D, Gd = gram_on_device(rows, nu, n)
    assert (Gd.cpu().numpy().astype(LD) == G).all()           # the device's G is the exact one
    model = SLIM(0.01, 0.01)
    whole = [x.cpu().numpy() for x in model.solve(D, Gd, nu)]
    ref = fitted(n, rows, 0.01, 0.01, 1e-4)
    assert whole[0].tobytes() == dense(ref, n).tobytes() and whole[2].tobytes() == ref.kkt.cpu().numpy().tobytes()
    for a, b in ranges:
        part = [x.cpu().numpy() for x in model.solve(D, Gd, nu, a, b)]
        assert part[0][:, a:b].tobytes() == whole[0][:, a:b].tobytes(), (a, b)
        for x, y in zip(part[1:], whole[1:]):
            assert x[a:b].tobytes() == y[a:b].tobytes(), (a, b)
        for x in part:                                        # nothing outside the range is written
            outside = np.ones(n, dtype=bool)
            outside[a:b] = False
            assert not (x[:, outside] if x.ndim == 2 else x[outside]).any(), (a, b)
    padded = torch.full((n, n + 5), 7.5, dtype=torch.float64, device=DEV)    # a leading dimension above n
    padded[:, :n] = Gd
    again = [x.cpu().numpy() for x in model.solve(D, padded[:, :n], nu)]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, whole))


def test_the_same_bytes_from_every_kind_of_log_and_from_two_fits_in_a_row():
    rows, _, _ = shape_log(65)
    first = fit(rows, 0.01, 0.01)
    want = table_bytes(first)
    assert want == table_bytes(fitted(65, rows, 0.01, 0.01, 1e-4))
    for kind in (as_arrow, as_device):
        assert table_bytes(fit(rows, 0.01, 0.01, kind=kind)) == want
    updates = first.n_updates
    first.fit(frame(*rows))
    assert table_bytes(first) == want and first.n_updates == updates


def test_seed_has_no_effect():
    rows, _, _ = shape_log(17)
    a, b = SLIM(0.01, 0.01, seed=1), SLIM(0.01, 0.01, seed=2)
    a.fit(frame(*rows))
    b.fit(frame(*rows))
    assert table_bytes(a) == table_bytes(b) and a._init_args["seed"] == 1


def test_similarity_frame_order_dtypes_and_an_item_without_interactions():
    n_users, n = 80, 20
    user, item, rel = SR.random_log(n_users, n, .2, 31, 3, untouched=(0, 9))
    model = fit((user, item, rel), 0.01, 0.01)
    S = dense(model, n)
    sim = model.similarity
    assert list(sim.columns) == ["item_idx_one", "item_idx_two", "similarity"]
    assert [str(t) for t in sim.dtypes] == ["int32", "int32", "float64"]
    r, c = np.nonzero(S)                                     # row-major: item_idx_one = i, item_idx_two = j, S[i, j] = w^(j)_i
    assert sim["item_idx_one"].tolist() == r.tolist() and sim["item_idx_two"].tolist() == c.tolist()
    assert sim["similarity"].tolist() == S[r, c].tolist() and (sim["similarity"] > 0).all()
    for it in (0, 9):
        assert it not in set(sim["item_idx_one"]) and it not in set(sim["item_idx_two"])
    off, col, val = model.similarity_device
    assert off.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float64
    assert model.n_sweeps.dtype == torch.int32 and model.kkt.dtype == torch.float64 and isinstance(model.n_updates, int)
    G = SR.exact_gram(SR.interactions(user, item, rel, n_users, n))
    check_certificate(model, G, n_users, 0.01, 0.01, 1e-4, "two untouched items")


def test_max_iter_one_with_a_tiny_tol_warns_and_counts():
    rows, G, nu = shape_log(65)
    model = SLIM(0.01, 0.01)
    model.tol, model.max_iter = 1e-15, 1
    with pytest.warns(RuntimeWarning, match=r"SLIM: (\d+) of 65 columns did not reach") as rec:
        model.fit(frame(*rows))
    assert model.n_not_converged > 0 and f"SLIM: {model.n_not_converged} of 65" in str(rec[0].message)
    sweeps, kkt = model.n_sweeps.cpu().numpy(), model.kkt.cpu().numpy()
    assert (sweeps == 1).all() and model.n_not_converged == int((kkt > 1e-15 * 0.01).sum())
    S = dense(model, 65)                                      # the reported certificate is still the certificate of what came out
    for j in range(65):
        v, r = SR.certificate(G, j, S[:, j], nu, 0.01, 0.01), SR.refresh_rounding(G, j, S[:, j], nu, 0.01, 0.01)
        assert abs(LD(kkt[j]) - np.max(np.abs(v))) <= np.max(r), j
    assert 0 < model.n_updates <= 65 * 64
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fit(rows, 0.01, 0.01)                                 # a converged fit does not warn


def test_a_large_lambda_gives_an_empty_table_after_one_sweep():
    rows, G, nu = shape_log(65)
    big = float(np.max(np.abs(G))) / nu + 1.0                 # nu lambda_ above every |q_i|: no coordinate ever moves
    model = fit(rows, 0.01, big)
    assert len(model.similarity) == 0 and model.similarity_device[1].numel() == 0 and model.n_updates == 0
    sweeps = model.n_sweeps.cpu().numpy()
    assert (sweeps[np.diag(G) != 0] == 1).all() and (sweeps[np.diag(G) == 0] == 0).all()
    assert not model.kkt.cpu().numpy().any() and model.n_not_converged == 0


def test_a_catalogue_above_the_cap_is_refused():
    log = {"user_idx": torch.tensor([0, 1], device=DEV), "item_idx": torch.tensor([0, N.SLIM_MAX_ITEMS], device=DEV)}
    with pytest.raises(ValueError, match=f"{N.SLIM_MAX_ITEMS + 1} items are out of range"):
        SLIM().fit(log)


# ------------------------------------------------------------------------------------------------- predictions
def close_lists(got, ref, scale):
    """[(j, score)] equal up to the rounding of a sum: scores within tol, ids equal except across a tie within tol"""
    tol = 64 * 2.0 ** -53 * scale
    assert len(got) == len(ref)
    ref_score = dict(ref)
    for (gj, gs), (rj, rs) in zip(got, ref):
        assert abs(gs - rs) <= tol
        assert gj == rj or abs(ref_score[gj] - rs) <= tol


@pytest.mark.parametrize("filter_seen", [True, False])
def test_predictions_equal_the_dense_product_under_the_tie_rule(filter_seen):
    n_items = 65
    (user, item, rel), _, n_users = shape_log(n_items)
    model = fitted(n_items, (user, item, rel), 0.01, 0.01, 1e-4)
    C = dense(model, n_items)
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
            full = cnt[int(u)] @ C                         # the dense product x_u S: the score of every listed item
            for j, s in got.get(int(u), []):
                assert abs(full[j] - s) <= 64 * 2.0 ** -53 * scale
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
            assert abs(got[(int(u), int(j))] - r) <= 64 * 2.0 ** -53 * scale
    near = model.get_nearest_items([3, 5], k=4)
    assert list(near.columns) == ["item_idx", "neighbour_item_idx", "similarity"]
    for i in (3, 5):
        kth = sorted(C[i][C[i] != 0], reverse=True)[:4]
        rows_i = near[near["item_idx"] == i]
        assert sorted(rows_i["similarity"], reverse=True) == kth
        assert all(C[i, int(j)] == s for j, s in zip(rows_i["neighbour_item_idx"], rows_i["similarity"]))


# ------------------------------------------------------------------------------------------------- neighbours
def test_the_other_neighbourhood_models_keep_their_bytes_beside_a_slim_fit():
    from replay_cql_amd.neighbour import ItemKNN
    rows, _, _ = shape_log(63)
    df = frame(*rows)

    def tables():
        knn, admm = ItemKNN(10), ADMMSLIM(0.5, 4, seed=3)
        admm.max_iteration = 3
        knn.fit(df)
        admm.fit(df)
        return [x.cpu().numpy().tobytes() for m in (knn, admm) for x in m.similarity_device]
    before = tables()
    fit(rows, 0.01, 0.01)
    assert tables() == before
