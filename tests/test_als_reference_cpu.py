"""The ALS yardstick (tests/als_reference.py) against answers worked by hand; no GPU, no package code."""
import numpy as np

import als_reference as R


def test_rank_one_closed_form():
    """one user with two entries at rank 1: x = b / (A + reg n_expl), every number written out"""
    F = np.array([[0.5], [2.0], [-1.0]], dtype=np.float32)            # three source rows
    side = (np.array([0, 2]), np.array([0, 1]), np.array([3.0, -1.0]))  # the row rates source 0 with 3, source 1 with -1
    alpha, reg = 0.5, 0.1
    G = 0.25 + 4.0 + 1.0
    # implicit: c = (1.5, 0.5); A = G + 1.5 * 0.25 + 0.5 * 4; b = (1 + 1.5) * 0.5 (only the positive rating); n_expl = 1
    A, b, ne = R.normal_equations(side, F, True, alpha, np.array([[G]]))[:3]
    assert A[0, 0, 0] == G + 0.375 + 2.0 and b[0, 0] == 1.25 and ne[0] == 1
    X, has = R.half_step(side, F, True, alpha, reg)
    assert has[0] == 1 and abs(X[0, 0] - 1.25 / (7.625 + 0.1)) < 1e-16
    # explicit: A = 0.25 + 4; b = 3 * 0.5 - 1 * 2; n_expl = 2
    A, b, ne = R.normal_equations(side, F, False, alpha)[:3]
    assert A[0, 0, 0] == 4.25 and b[0, 0] == -0.5 and ne[0] == 2
    X, _ = R.half_step(side, F, False, alpha, reg)
    assert abs(X[0, 0] - (-0.5) / (4.25 + 0.2)) < 1e-16


def test_row_without_entries_has_no_factor():
    F = np.ones((2, 3), dtype=np.float32)
    side = (np.array([0, 0, 1]), np.array([1]), np.array([1.0]))
    X, has = R.half_step(side, F, True, 1.0, 0.1)
    assert has.tolist() == [0, 1] and not X[0].any() and X[1].any()


def test_explicit_reproduces_an_exact_rank_one_matrix():
    """3 x 2, fully observed, M = p q^T, reg = 0: from any user factors that are not orthogonal to p the first item step
    gives q up to scale and the user step the matching p, so U V^T = M"""
    p, q = np.array([1.0, 2.0, -0.5]), np.array([3.0, 0.25])
    M = np.outer(p, q)
    user, item = np.repeat(np.arange(3), 2), np.tile(np.arange(2), 3)
    U0 = np.array([[0.5], [0.25], [1.0]])
    (U, V), = R.fit(user, item, M.ravel(), 3, 2, U0, False, 1.0, 0.0, 1, store=np.float64)
    assert np.allclose(U @ V.T, M, rtol=0, atol=1e-14)


def test_implicit_objective_does_not_increase():
    rng = np.random.default_rng(5)
    n_users, n_items, r = 12, 9, 3
    pairs = [(u, i) for u in range(n_users) for i in range(n_items) if rng.random() < 0.4 or i == u % n_items]
    user, item = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    rel = rng.integers(1, 6, len(pairs)).astype(np.float64)
    rel[rng.random(len(pairs)) < 0.15] *= -1.0                        # some negatives: confidence without preference
    for u in range(n_users):                                          # every user and item keeps a positive rating
        rel[np.nonzero(user == u)[0][0]] = abs(rel[np.nonzero(user == u)[0][0]])
    for i in range(n_items):
        if not (rel[item == i] > 0).any():
            rel[np.nonzero(item == i)[0][0]] *= -1.0
    U0 = rng.normal(size=(n_users, r))
    U0 /= np.linalg.norm(U0, axis=1, keepdims=True)
    steps = R.fit(user, item, rel, n_users, n_items, U0, True, 1.0, 0.1, 5, store=np.float64)
    obj = [R.implicit_objective(user, item, rel, U, V, 1.0, 0.1) for U, V in steps]
    for a, b in zip(obj, obj[1:]):
        assert b <= a * (1.0 + 1e-12), obj
    assert obj[-1] < obj[0]


def test_dyadic_inputs_sum_the_same_in_any_order():
    """the inputs of the bit-for-bit GPU test: factors k / 64 within +-2, ratings k / 4 within +-8, alpha = 0.5, rows of
    up to 2^13 entries: every product and every partial sum is exact in float64"""
    rng = np.random.default_rng(11)
    F = (rng.integers(-128, 129, (50, 5)) / 64.0).astype(np.float32)
    n = 1 << 13
    side = (np.array([0, n]), rng.integers(0, 50, n), rng.integers(-32, 33, n) / 4.0)
    G, Gs, exact_g = R.gram(F)
    assert exact_g
    for implicit in (True, False):
        out = R.normal_equations(side, F, implicit, 0.5, G, Gs)
        assert out[-1], implicit
    general = rng.normal(size=(50, 5)).astype(np.float32)
    assert not R.normal_equations(side, general, True, 0.5, R.gram(general)[0])[-1]


def test_tolerances():
    assert R.tolerance("sum", n=6, n_G=0, abs_terms=2.0) == 16 * 2.0 ** -53
    t = R.tolerance("solve", r=2, kappa=10.0, x=np.array([3.0, 4.0]))
    assert np.allclose(t, 2 * 2 * 7 * 2.0 ** -53 * 10 * 5 + 2.0 ** -24 * np.array([3.0, 4.0]), rtol=1e-15)
    assert R.tolerance("score", r=10, abs_dot=1.5) == 15 * 2.0 ** -24
