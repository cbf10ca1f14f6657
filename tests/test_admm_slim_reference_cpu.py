"""The yardstick tests/admm_slim_reference.py checked on its own, without a GPU: against answers worked by hand and in
exact rational arithmetic (tests/golden/admm_slim_known_answers.json), against numpy.linalg.inv, and against five
plausible mistakes, each of which it must tell from the normative text.  The whole-fit cases are run in float64 and in
longdouble: the iteration counts, the rho sequences and the spread between the two are the ones stored for the GPU
test."""
import json
from pathlib import Path

import numpy as np
import pytest

import admm_slim_reference as AR

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "admm_slim_known_answers.json").read_text())
LD = np.longdouble


@pytest.mark.parametrize("name", ["iteration_2x2", "iteration_3x3"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_one_iteration_equals_the_worked_answer(name, dtype):
    case = GOLDEN[name]
    W, P, C, Gamma = (np.array(case[k], dtype=dtype) for k in ("W", "P", "C", "Gamma"))
    B, C1, G1, norms = AR.iteration(W, P, C, Gamma, dtype(case["rho"]), dtype(case["lambda_1"]))
    assert B.tolist() == case["B"] and C1.tolist() == case["C1"] and G1.tolist() == case["Gamma1"]   # dyadic: exact
    assert [float(x * x) for x in norms] == pytest.approx(case["squares"], rel=1e-15)
    by_rows = AR.iteration(W, P, C, Gamma, dtype(case["rho"]), dtype(case["lambda_1"]), rows=True)
    if name == "iteration_3x3":                            # the 2 x 2 case has v = (1, 1): rows and columns agree there
        assert by_rows[1].tolist() != case["C1"]


def test_the_inverse_and_the_gram_matrix_of_duplicated_rows():
    case = GOLDEN["inverse_2x2"]
    for dtype in (np.float64, np.longdouble):
        got = AR.spd_inverse(np.array(case["A"], dtype=dtype))
        assert np.allclose((3 * got).astype(np.float64), case["times_3"], rtol=0, atol=1e-15)
    rs = np.random.RandomState(0)
    X = rs.rand(40, 12)
    A = X.T @ X + 0.5 * np.eye(12)
    assert np.allclose(AR.spd_inverse(A), np.linalg.inv(A), rtol=1e-11, atol=0)
    assert np.abs(AR.spd_inverse(A.astype(LD)) @ A.astype(LD) - np.eye(12)).max() < 1e-16
    with pytest.raises(ValueError):
        AR.spd_inverse(-np.eye(2))
    case = GOLDEN["gram_duplicates"]
    X = AR.interactions(case["user"], case["item"], case["relevance"])
    assert X.tolist() == case["X"] and (X.T @ X).tolist() == case["G"]
    last = AR.interactions(case["user"], case["item"], case["relevance"], sum_duplicates=False)
    assert (last.T @ last).tolist() == case["G_last_wins"] != case["G"]


def test_the_draws_are_three_rand_calls_in_the_order_b_c_gamma():
    rs = np.random.RandomState(11)
    want = [rs.rand(5, 5) for _ in range(3)]
    got = AR.draws(5, 11)
    assert all((a == b).all() for a, b in zip(got, want))
    rs = np.random.RandomState(11)                         # the first draw made in chunks and dropped: the same C and Gamma
    rs.random_sample(13), rs.random_sample(12)
    assert (rs.rand(5, 5) == want[1]).all() and (rs.rand(5, 5) == want[2]).all()
    swapped = AR.draws(5, 11, c_first=True)
    assert (swapped[1] == want[0]).all() and (swapped[0] == want[1]).all()


def duplicated_case():
    n_users, n_items, p, lam1, lam2, seed, R = AR.CASES[0]
    user, item, rel = AR.random_log(n_users, n_items, p, seed, R)
    user, item, rel = np.concatenate([user, user[:30]]), np.concatenate([item, item[:30]]), np.concatenate([rel, rel[:30] + 1])
    return user, item, rel, (n_users, n_items, lam1, lam2, seed)


@pytest.mark.parametrize("mistake", AR.MISTAKES)
def test_each_plausible_mistake_changes_the_result(mistake):
    user, item, rel, (n_users, n_items, lam1, lam2, seed) = duplicated_case()
    X = AR.interactions(user, item, rel, n_users, n_items)
    right = AR.fit(X, lam1, lam2, seed)
    assert len(set(right["rho"])) > 1                      # rho changes, so a W rebuilt from it differs
    if mistake == "no_dup_sum":
        wrong = AR.fit(AR.interactions(user, item, rel, n_users, n_items, sum_duplicates=False), lam1, lam2, seed)
    else:
        wrong = AR.fit(X, lam1, lam2, seed, mistake=mistake)
    gap = np.abs(wrong["C"] - right["C"]).max()
    assert gap > 1e-6 * np.abs(right["C"]).max(), (mistake, gap)
    again = AR.fit(X, lam1, lam2, seed)
    assert again["C"].tobytes() == right["C"].tobytes() and again["rho"] == right["rho"]


@pytest.mark.parametrize("index", range(len(AR.CASES)))
def test_whole_fit_cases_in_float64_and_longdouble(index):
    stored = GOLDEN["whole_fit"][index]
    assert stored["case"] == list(AR.CASES[index])
    _, f64 = AR.case_fit(AR.CASES[index])
    _, fld = AR.case_fit(AR.CASES[index], dtype=LD)
    assert f64["iterations"] == fld["iterations"] == stored["iterations"]
    assert f64["rho"] == fld["rho"] == stored["rho"]
    for f in (f64, fld):                                   # no comparison near a tie: a flipped branch is never rounding
        assert f["branch_margin"] >= 1e-2 and f["stop_margin"] >= 3e-4
    spread = float(np.abs(f64["C"].astype(LD) - fld["C"]).max())
    top = float(np.abs(f64["C"]).max())
    print(f"case {index}: iterations {f64['iterations']}, rho {min(f64['rho'][1:])}..{max(f64['rho'][1:])}, spread {spread:.3g}, "
          f"max |C| {top:.3g}, pattern flips {int(((f64['C'] != 0) != (fld['C'] != 0)).sum())}")
    assert 1e-18 < spread < 2e-15 and stored["spread"] / 4 <= spread <= stored["spread"] * 4
    assert top == pytest.approx(stored["max_abs_C"], rel=1e-9)
    flipped = (f64["C"] != 0) != (fld["C"] != 0)
    assert flipped.sum() <= 16 and np.abs(f64["C"][flipped]).max(initial=0) <= 32 * spread


def test_the_stopping_rule_and_the_iteration_cap():
    n_users, n_items, p, lam1, lam2, seed, R = AR.CASES[0]
    user, item, rel = AR.random_log(n_users, n_items, p, seed, R)
    X = AR.interactions(user, item, rel, n_users, n_items)
    assert AR.fit(X, lam1, lam2, seed, max_iteration=0)["iterations"] == 0
    one = AR.fit(X, lam1, lam2, seed, max_iteration=1)
    assert one["iterations"] == 1 and len(one["rho"]) == 2 and (one["C"] != 0).sum() < n_items * n_items
    full = AR.fit(X, lam1, lam2, seed)
    r_p, r_d, e_p, e_d = full["residuals"]
    assert r_p <= e_p and r_d <= e_d and full["iterations"] < 100
