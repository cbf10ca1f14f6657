"""Writes tests/golden/slim_known_answers.json: what sklearn's ElasticNet gives on the golden logs of
tests/slim_reference.py, once at the reference's exact settings (replay/models/slim.py: max_iter 5000, tol 1e-4,
selection="random", seeded) and once tight (tol 1e-14, selection="cyclic"), with the measured spread between the two, and
the table of cqlrec_slim_fit_ws_bytes.  Needs scikit-learn and scipy and the built library; run on a CPU:

    python tests/golden/make_slim_golden.py

The tests read only the JSON."""
import json
import sys
import warnings
from pathlib import Path

import numpy as np
import scipy
import sklearn
from scipy.sparse import csc_matrix
from sklearn.linear_model import ElasticNet

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import slim_reference as SR  # noqa: E402
from replay_cql_amd import _native as N  # noqa: E402

SEED = 42


def sklearn_fit(X, beta, lambda_, **settings):
    """S [n, n] with S[:, j] = the coefficients of column j regressed on X with column j zeroed, as the reference does"""
    n = X.shape[1]
    alpha = beta + lambda_
    model = ElasticNet(alpha=alpha, l1_ratio=lambda_ / alpha, fit_intercept=False, positive=True, **settings)
    S = np.zeros((n, n))
    for j in range(n):
        A = X.copy()
        A[:, j] = 0
        with warnings.catch_warnings():
            # a fit that does not converge must not be recorded; on an all-zero target sklearn's tolerance is 0 and it
            # warns about a gap of 0 at the zero solution
            warnings.simplefilter("error" if X[:, j].any() else "ignore")
            model.fit(csc_matrix(A), X[:, j])
        S[:, j] = model.coef_
    return S


def main():
    out = {"sklearn": sklearn.__version__, "scipy": scipy.__version__, "numpy": np.__version__, "seed": SEED,
           "default_settings": {"max_iter": 5000, "tol": 1e-4, "selection": "random", "random_state": SEED},
           "tight_settings": {"max_iter": 1000000, "tol": 1e-14, "selection": "cyclic"}, "cases": {}}
    for name, spec in SR.GOLDEN_LOGS.items():
        user, item, rel = SR.random_log(*spec)
        X = SR.interactions(user, item, rel, spec[0], spec[1])
        case = {"spec": [list(x) if isinstance(x, tuple) else x for x in spec], "user": user.tolist(), "item": item.tolist(),
                "relevance": rel.tolist(), "fits": []}
        for beta, lambda_ in SR.GOLDEN_PARAMS:
            default = sklearn_fit(X, beta, lambda_, max_iter=5000, random_state=SEED, selection="random")
            tight = sklearn_fit(X, beta, lambda_, max_iter=1000000, tol=1e-14, selection="cyclic")
            diff = default - tight
            case["fits"].append({"beta": beta, "lambda_": lambda_, "default": default.tolist(), "tight": tight.tolist(),
                                 "spread_max": float(np.abs(diff).max()),
                                 "spread_l2": float(np.sqrt((diff * diff).sum(axis=0)).max()),
                                 "spread_l1": float(np.abs(diff).sum(axis=0).max()),
                                 "support_differences": int(((default > 0) != (tight > 0)).sum())})
            print(name, beta, lambda_, {k: v for k, v in case["fits"][-1].items() if k.startswith(("spread", "support"))})
        out["cases"][name] = case
    lib = N.load()
    cap = N.SLIM_MAX_ITEMS
    out["cap"] = cap
    out["ws_bytes"] = {str(n): int(lib.cqlrec_slim_fit_ws_bytes(n)) for n in (1, 64, 1025, 16384, cap + 1)}
    path = ROOT / "tests" / "golden" / "slim_known_answers.json"
    path.write_text(json.dumps(out) + "\n")
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
