"""A numpy-only yardstick of ADMM SLIM, written from the normative text of DESIGN.md section 3.14 (not from any
implementation), in a floating-point type of the caller's choice: numpy.float64, or numpy.longdouble to measure what
rounding does to a fit.

    X      users x items, duplicated (user, item) rows SUMMED
    G      = X^T X;  rho_0 = lambda_2;  W = (G + (lambda_2 + rho_0) I)^-1, computed once;  P = W G
    draws  RandomState(seed): three rand(n, n) in the order B, C, Gamma
    loop   while (r_p > eps_p or r_d > eps_d) and it < max_iteration, from r_p = |B - C|, r_d = |rho C|, eps = 0:
             T = P + W (rho C - Gamma);  v_j = T_jj / W_jj;  B_ij = T_ij - W_ij v_j      (v scales COLUMNS)
             S = B + Gamma / rho;  c = lambda_1 / rho;  C' = max(S - c, 0) - max(-S - c, 0)
             Gamma' = Gamma + rho (B - C')
             r_p = |B - C'|;  r_d = |rho (C' - C)|
             eps_p = eps_abs n + eps_rel max(|B|, |C'|);  eps_d = eps_abs n + eps_rel |Gamma'|
             rho <- rho * multiplicator if r_p > threshold r_d, else rho / multiplicator if threshold r_p < r_d
    table  the non-zeros of the final C, row-major

`mistake` plants one plausible error, for the tests that show the yardstick tells them apart:
    "rows"  v scales rows;  "rebuild_w"  W is recomputed from the current rho;  "no_dup_sum"  a duplicated (user, item)
    keeps its last value;  "c_first"  C is drawn before B;  "rho_first"  rho is updated before Gamma'."""
import numpy as np

MISTAKES = ("rows", "rebuild_w", "no_dup_sum", "c_first", "rho_first")
DEFAULTS = dict(threshold=5, multiplicator=2, eps_abs=1.0e-3, eps_rel=1.0e-3, max_iteration=100)


def interactions(user, item, relevance, n_users=None, n_items=None, dtype=np.float64, sum_duplicates=True):
    user, item = np.asarray(user, dtype=np.int64), np.asarray(item, dtype=np.int64)
    n_users = int(user.max()) + 1 if n_users is None else n_users
    n_items = int(item.max()) + 1 if n_items is None else n_items
    X = np.zeros((n_users, n_items), dtype=dtype)
    if sum_duplicates:
        np.add.at(X, (user, item), np.asarray(relevance, dtype=dtype))
    else:
        X[user, item] = np.asarray(relevance, dtype=dtype)
    return X


def fro(x):
    return np.sqrt(np.sum(x * x))


def spd_inverse(A):
    """the inverse of a symmetric positive definite matrix in A's own type: Cholesky, two triangular solves"""
    n, dt = A.shape[0], A.dtype
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise ValueError("not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.zeros_like(A)                                  # L Y = I
    eye = np.eye(n, dtype=dt)
    for i in range(n):
        Y[i] = (eye[i] - L[i, :i] @ Y[:i]) / L[i, i]
    Xi = np.zeros_like(A)                                 # L^T X = Y
    for i in range(n - 1, -1, -1):
        Xi[i] = (Y[i] - L[i + 1:, i] @ Xi[i + 1:]) / L[i, i]
    return Xi


def draws(n, seed, c_first=False):
    rs = np.random.RandomState(seed)
    a, b, g = rs.rand(n, n), rs.rand(n, n), rs.rand(n, n)
    return (b, a, g) if c_first else (a, b, g)


def iteration(W, P, C, Gamma, rho, lambda_1, rows=False):
    """(B, C', Gamma', the five norms |B - C'|, |C' - C|, |B|, |C'|, |Gamma'|) of one iteration at rho"""
    T = P + W @ (rho * C - Gamma)
    v = np.diag(T) / np.diag(W)
    B = T - (W * v[:, None] if rows else W * v[None, :])
    S = B + Gamma / rho
    c = lambda_1 / rho
    zero = np.zeros((), dtype=S.dtype)
    C1 = np.maximum(S - c, zero) - np.maximum(-S - c, zero)
    G1 = Gamma + rho * (B - C1)
    return B, C1, G1, (fro(B - C1), fro(C1 - C), fro(B), fro(C1), fro(G1))


def _margin(a, b):
    return float(abs(a - b) / max(abs(a), abs(b))) if max(abs(a), abs(b)) > 0 else 1.0


def fit(X, lambda_1, lambda_2, seed, dtype=np.float64, mistake=None, keep_states=(), **kw):
    """dict: C, Gamma, rho (the sequence, rho[0] = lambda_2), iterations, residuals (r_p, r_d, eps_p, eps_d), branch_margin
    and stop_margin (the smallest relative distance of an evaluated comparison from a tie), states {it: (W, P, C, Gamma,
    rho) BEFORE iteration it + 1} for the `it` in keep_states"""
    assert mistake is None or mistake in MISTAKES
    o = dict(DEFAULTS, **kw)
    X = np.asarray(X, dtype=dtype)
    n = X.shape[1]
    lam1, lam2 = dtype(lambda_1), dtype(lambda_2)
    thr, mul = dtype(o["threshold"]), dtype(o["multiplicator"])
    eps_abs, eps_rel = dtype(o["eps_abs"]), dtype(o["eps_rel"])
    G = X.T @ X
    rho = lam2
    eye = np.eye(n, dtype=dtype)
    W = spd_inverse(G + (lam2 + rho) * eye)
    P = W @ G
    B, C, Gamma = (m.astype(dtype) for m in draws(n, seed, c_first=mistake == "c_first"))
    r_p, r_d = fro(B - C), fro(rho * C)
    e_p = e_d = dtype(0)
    it, rhos, states = 0, [float(rho)], {}
    branch_margin = stop_margin = 1.0

    def go_on():
        nonlocal stop_margin
        stop_margin = min(stop_margin, _margin(r_p, e_p))
        if r_p > e_p:
            return True
        stop_margin = min(stop_margin, _margin(r_d, e_d))
        return bool(r_d > e_d)

    while it < o["max_iteration"] and go_on():
        if it in keep_states:
            states[it] = (W.copy(), P.copy(), C.copy(), Gamma.copy(), float(rho))
        it += 1
        if mistake == "rebuild_w":
            W = spd_inverse(G + (lam2 + rho) * eye)
            P = W @ G
        B, C1, G1, s = iteration(W, P, C, Gamma, rho, lam1, rows=mistake == "rows")
        r_p, r_d = s[0], rho * s[1]
        branch_margin = min(branch_margin, _margin(r_p, thr * r_d))
        rho_next = rho
        if r_p > thr * r_d:
            rho_next = rho * mul
        else:
            branch_margin = min(branch_margin, _margin(thr * r_p, r_d))
            if thr * r_p < r_d:
                rho_next = rho / mul
        if mistake == "rho_first":
            G1 = Gamma + rho_next * (B - C1)
        e_p = eps_abs * n + eps_rel * max(s[2], s[3])
        e_d = eps_abs * n + eps_rel * fro(G1)
        C, Gamma, rho = C1, G1, rho_next
        rhos.append(float(rho))
    return {"C": C, "Gamma": Gamma, "W": W, "P": P, "rho": rhos, "iterations": it,
            "residuals": (float(r_p), float(r_d), float(e_p), float(e_d)), "branch_margin": branch_margin,
            "stop_margin": stop_margin, "states": states}


def random_log(n_users, n_items, p, seed, R):
    """the rows (user, item, relevance) of the whole-fit cases: RandomState(100 + seed), an entry present with probability
    p, its relevance uniform in 1..R"""
    rs = np.random.RandomState(100 + seed)
    present = rs.rand(n_users, n_items) < p
    rel = rs.randint(1, R + 1, size=(n_users, n_items))
    user, item = np.nonzero(present)
    return user.astype(np.int64), item.astype(np.int64), rel[present].astype(np.float64)


# users, items, p, lambda_1, lambda_2, seed, R
CASES = [(60, 17, .3, .5, 4, 1, 1), (200, 48, .15, .5, 4, 2, 1), (300, 80, .1, 1, 8, 3, 3), (500, 130, .08, 5, 5000, 4, 1),
         (400, 65, .1, .25, 2, 5, 5), (200, 48, .15, 1e-3, 1e-3, 6, 1)]


def case_fit(case, dtype=np.float64, **kw):
    n_users, n_items, p, lam1, lam2, seed, R = case
    user, item, rel = random_log(n_users, n_items, p, seed, R)
    X = interactions(user, item, rel, n_users, n_items, dtype=dtype)
    return (user, item, rel), fit(X, lam1, lam2, seed, dtype=dtype, **kw)
