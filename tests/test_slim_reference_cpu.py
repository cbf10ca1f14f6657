"""The SLIM yardstick (tests/slim_reference.py) against what sklearn's ElasticNet recorded in
tests/golden/slim_known_answers.json (made by tests/golden/make_slim_golden.py; sklearn is not needed here).

Every bound is derived in slim_reference.py, none is fitted:
  certificate   |v_i| <= tol lambda_ + r_i, r the rounding of the float64 refresh and certificate
  beta > 0      |w - w'|_2 <= (|v|_2 + |v'|_2) / beta                      (strong convexity)
  beta = 0      F(w) - F(w') <= (|v|_inf + |v'|_inf) |w - w'|_1 + the rounding of the two evaluations of F
The recorded solutions at the reference's own settings (tol 1e-4, random order) are NOT at the minimiser: they lie
within the recorded spread of the tight ones, which is what this file documents (up to 1.9e-3 per column in l2)."""
import json
from pathlib import Path

import numpy as np
import pytest

import slim_reference as SR

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "slim_known_answers.json").read_text())
LD = np.longdouble
TOL = 1e-9
_CACHE = {}


def case(name):
    if name not in _CACHE:
        c = GOLDEN["cases"][name]
        spec = SR.GOLDEN_LOGS[name]
        user, item, rel = SR.random_log(*spec)
        assert (user.tolist(), item.tolist(), rel.tolist()) == (c["user"], c["item"], c["relevance"])
        X = SR.interactions(user, item, rel, spec[0], spec[1])
        G = SR.exact_gram(X)
        assert (G == (X.T @ X).astype(LD)).all()                  # integer data: float64 holds G exactly
        _CACHE[name] = (X, G, spec[0])
    return _CACHE[name]


def yardstick(name, index, dtype=np.float64):
    key = (name, index, dtype)
    if key not in _CACHE:
        _, G, nu = case(name)
        beta, lambda_ = SR.GOLDEN_PARAMS[index]
        _CACHE[key] = SR.fit(G, nu, beta, lambda_, tol=TOL, dtype=dtype)
    return _CACHE[key]


CASES = [(name, index) for name in SR.GOLDEN_LOGS for index in range(len(SR.GOLDEN_PARAMS))]


def test_the_golden_file_is_what_the_maker_describes():
    assert GOLDEN["default_settings"] == {"max_iter": 5000, "tol": 1e-4, "selection": "random", "random_state": GOLDEN["seed"]}
    assert GOLDEN["tight_settings"]["tol"] == 1e-14 and GOLDEN["tight_settings"]["selection"] == "cyclic"
    assert GOLDEN["sklearn"] and sorted(GOLDEN["cases"]) == sorted(SR.GOLDEN_LOGS)
    for name, c in GOLDEN["cases"].items():
        assert [(f["beta"], f["lambda_"]) for f in c["fits"]] == SR.GOLDEN_PARAMS
        assert max(c["item"]) + 1 <= 33
    dup = GOLDEN["cases"]["duplicates"]
    pairs = list(zip(dup["user"], dup["item"]))
    assert len(set(pairs)) < len(pairs) and 7 not in dup["item"]
    assert set(GOLDEN["cases"]["binary"]["relevance"]) == {1.0} and set(GOLDEN["cases"]["ratings"]["relevance"]) == {1.0, 2.0, 3.0, 4.0, 5.0}


@pytest.mark.parametrize("name,index", CASES)
def test_certificate_of_the_yardstick(name, index):
    _, G, nu = case(name)
    beta, lambda_ = SR.GOLDEN_PARAMS[index]
    S, sweeps, kkt, updates = yardstick(name, index)
    n = len(G)
    assert (S >= 0).all() and (np.diag(S) == 0).all()
    worst = 0.0
    for j in range(n):
        v = SR.certificate(G, j, S[:, j], nu, beta, lambda_)
        r = SR.refresh_rounding(G, j, S[:, j], nu, beta, lambda_)
        assert (np.abs(v) <= LD(TOL) * LD(lambda_) + r).all(), j
        assert abs(LD(kkt[j]) - np.max(np.abs(v))) <= np.max(r), j
        worst = max(worst, float(np.max(np.abs(v))))
        if G[j, j] == 0:
            assert sweeps[j] == 0 and updates[j] == 0 and not S[:, j].any()
        else:
            assert 1 <= sweeps[j] < 5000
    print(f"{name} {SR.GOLDEN_PARAMS[index]}: worst certificate {worst:.3g}, sweeps median {int(np.median(sweeps))} max {int(sweeps.max())}, "
          f"updates {int(updates.sum())}")


@pytest.mark.parametrize("name,index", CASES)
def test_yardstick_against_the_recorded_sklearn_solutions(name, index):
    _, G, nu = case(name)
    beta, lambda_ = SR.GOLDEN_PARAMS[index]
    rec = GOLDEN["cases"][name]["fits"][index]
    tight, default = np.array(rec["tight"]), np.array(rec["default"])
    S = yardstick(name, index)[0]
    worst = [0.0, 0.0]
    for j in range(len(G)):
        if beta > 0:
            dist, bound = SR.distance_and_bound(G, j, S[:, j], tight[:, j], nu, beta, lambda_)
            assert dist <= bound, j
            worst[0] = max(worst[0], float(dist))
            far = np.sqrt(np.sum((S[:, j].astype(LD) - default[:, j]) ** 2))
            assert far <= LD(rec["spread_l2"]) + bound, j
            worst[1] = max(worst[1], float(far))
        else:
            for a, b in ((S[:, j], tight[:, j]), (tight[:, j], S[:, j])):
                gap, bound = SR.objective_gap_and_bound(G, j, a, b, nu, beta, lambda_)
                assert gap <= bound, j
            gap, bound = SR.objective_gap_and_bound(G, j, S[:, j], default[:, j], nu, beta, lambda_)
            assert gap <= bound, j
    # the recorded spread is what the maker measured between sklearn's own two settings
    diff = default - tight
    assert float(np.sqrt((diff * diff).sum(axis=0)).max()) == rec["spread_l2"] and float(np.abs(diff).max()) == rec["spread_max"]
    print(f"{name} {SR.GOLDEN_PARAMS[index]}: to the tight solution {worst[0]:.3g}, to the default one {worst[1]:.3g} "
          f"(recorded spread {rec['spread_l2']:.3g})")


def test_float64_and_longdouble_descents_agree_within_the_bound():
    for name, index in (("binary", 0), ("duplicates", 1)):
        _, G, nu = case(name)
        beta, lambda_ = SR.GOLDEN_PARAMS[index]
        S, SL = yardstick(name, index)[0], yardstick(name, index, LD)[0]
        for j in range(len(G)):
            dist, bound = SR.distance_and_bound(G, j, S[:, j], SL[:, j], nu, beta, lambda_)
            assert dist <= bound


def test_screening_gives_the_iterates_of_the_plain_loop():
    _, G, nu = case("ratings")
    for index in range(len(SR.GOLDEN_PARAMS)):
        beta, lambda_ = SR.GOLDEN_PARAMS[index]
        for j in (0, 16, 32):
            a = SR.descend(G, j, nu, beta, lambda_, tol=1e-6)
            b = SR.descend_plain(G, j, nu, beta, lambda_, tol=1e-6)
            assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


def test_the_certificate_tells_a_wrong_solution():
    _, G, nu = case("binary")
    beta, lambda_ = SR.GOLDEN_PARAMS[0]
    w = yardstick("binary", 0)[0][:, 3].copy()
    k = int(np.argmax(w))
    for wrong in (w * 1.01, np.where(np.arange(len(w)) == k, 0.0, w)):
        v = SR.certificate(G, 3, wrong, nu, beta, lambda_)
        assert np.max(np.abs(v)) > 100 * TOL * lambda_
    free = w.copy()
    free[3] = 0.5                                            # the constraint w_j = 0 is the caller's: v_j is 0 by definition
    assert SR.certificate(G, 3, free, nu, beta, lambda_)[3] == 0


def test_max_iter_stops_the_descent_and_a_large_lambda_gives_zero_after_one_sweep():
    _, G, nu = case("ratings")
    w, sweeps, kkt, updates = SR.descend(G, 5, nu, 0.01, 0.01, tol=1e-15, max_iter=1)
    assert sweeps == 1 and kkt > 1e-15 * 0.01 and updates > 0
    big = float(np.max(np.abs(G))) / nu + 1.0
    w, sweeps, kkt, updates = SR.descend(G, 5, nu, 0.01, big)
    assert not w.any() and sweeps == 1 and kkt == 0 and updates == 0
