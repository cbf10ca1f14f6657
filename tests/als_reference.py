"""numpy / float64 yardstick of DESIGN.md section 3.10 (ALS): math.fsum for every sum, numpy.linalg.solve for the solve.
Nothing here imports the package.  A side is (offsets int64 [n_dst + 1], src int [nnz], rating float64 [nnz]) and F the
source factors, float32 [n_src, r]; `tolerance` holds every bound the GPU tests assert."""
import math

import numpy as np

PIECE = 1024            # CQLREC_ALS_PIECE, restated: test_als_host.py compares it with the header
EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24


def tolerance(kind, **kw):
    """sum:    (n + n_G + 2) 2^-53 abs_terms -- an element of A, b or G against its fsum; n the row's entries, n_G the
               source rows of G (0 without G), abs_terms the sum of the absolute terms of that element
       solve:  2 r (3r + 1) 2^-53 kappa ||x||_2 + 2^-24 |x_i| -- the Cholesky backward-error bound, then the fp32 store
       score:  r 2^-24 abs_dot -- an fp32 fma chain of r terms against the fp64 dot, abs_dot = sum |x_k y_k|"""
    if kind == "sum":
        return (kw["n"] + kw["n_G"] + 2) * EPS64 * kw["abs_terms"]
    if kind == "solve":
        r = kw["r"]
        return 2.0 * r * (3 * r + 1) * EPS64 * kw["kappa"] * np.linalg.norm(kw["x"]) + EPS32 * np.abs(kw["x"])
    if kind == "score":
        return kw["r"] * EPS32 * kw["abs_dot"]
    raise ValueError(kind)


def _fsum_cols(T):
    """fsum over axis 0 of a 2-d array"""
    if T.shape[0] == 0:
        return np.zeros(T.shape[1])
    return np.array([math.fsum(col) for col in T.T.tolist()], dtype=np.float64)     # lists: fsum reads them fastest


def _order_free(T):
    """every column of T sums to the same float64 front to back and back to front (cumsum adds strictly in order)"""
    if T.shape[0] == 0:
        return True
    return bool(np.array_equal(np.cumsum(T, axis=0)[-1], np.cumsum(T[::-1], axis=0)[-1]))


def gram(F):
    """(G, sum of absolute terms, sums are order-free) of F^T F"""
    Y = np.asarray(F, dtype=np.float64)
    r = Y.shape[1]
    G, S, exact = np.zeros((r, r)), np.zeros((r, r)), True
    for i in range(r):
        T = Y[:, i:i + 1] * Y[:, :i + 1]
        G[i, :i + 1] = G[:i + 1, i] = _fsum_cols(T)
        S[i, :i + 1] = S[:i + 1, i] = _fsum_cols(np.abs(T))
        exact = exact and _order_free(T)
    return G, S, exact


def row_terms(side, F, row, implicit, alpha):
    """(c, w, Y, n_expl) of a destination row: the weights of the outer products, of b, and the source rows"""
    off, src, rating = side
    a, e = int(off[row]), int(off[row + 1])
    rho = np.asarray(rating[a:e], dtype=np.float64)
    Y = np.asarray(F, dtype=np.float64)[np.asarray(src[a:e], dtype=np.int64)]
    if implicit:
        c = alpha * np.abs(rho)
        w = np.where(rho > 0, 1.0 + c, 0.0)
        return c, w, Y, int((rho > 0).sum())
    return np.ones_like(rho), rho, Y, len(rho)


def normal_equations(side, F, implicit, alpha, G=None, G_abs=None, rows=None):
    """A [n, r, r] (G included when given, the regulariser not), b [n, r], n_expl [n], the sums of absolute terms of A
    and of b, and whether every sum came out the same in two different orders"""
    n_dst, r = len(side[0]) - 1, np.asarray(F).shape[1]
    rows = range(n_dst) if rows is None else rows
    A, b, ne = np.zeros((len(rows), r, r)), np.zeros((len(rows), r)), np.zeros(len(rows), dtype=np.int32)
    SA, Sb, exact = np.zeros_like(A), np.zeros_like(b), True
    for pos, row in enumerate(rows):
        c, w, Y, ne[pos] = row_terms(side, F, row, implicit, alpha)
        cY = c[:, None] * Y
        for i in range(r):
            T = cY[:, i:i + 1] * Y[:, :i + 1]
            A[pos, i, :i + 1] = A[pos, :i + 1, i] = _fsum_cols(T)
            SA[pos, i, :i + 1] = SA[pos, :i + 1, i] = _fsum_cols(np.abs(T))
            exact = exact and _order_free(T)
        Tb = w[:, None] * Y
        b[pos], Sb[pos] = _fsum_cols(Tb), _fsum_cols(np.abs(Tb))
        exact = exact and _order_free(Tb)
        if implicit and G is not None:
            exact = exact and bool(np.array_equal((A[pos] + G) - G, A[pos]))
            A[pos] = A[pos] + G
            if G_abs is not None:
                SA[pos] = SA[pos] + G_abs
    return A, b, ne, SA, Sb, exact


def solve(A, b, reg, n_expl):
    return np.linalg.solve(A + reg * float(n_expl) * np.eye(A.shape[0]), b)


def kappa2(A, reg, n_expl):
    return float(np.linalg.cond(A + reg * float(n_expl) * np.eye(A.shape[0]), 2))


def half_step(side, F, implicit, alpha, reg):
    """(X float64 [n_dst, r], has_factor [n_dst]): a row without entries has no factor and a zero row"""
    n_dst, r = len(side[0]) - 1, np.asarray(F).shape[1]
    G = gram(F)[0] if implicit else None
    A, b, ne = normal_equations(side, F, implicit, alpha, G)[:3]
    X, has = np.zeros((n_dst, r)), np.zeros(n_dst, dtype=np.uint8)
    for row in range(n_dst):
        if side[0][row + 1] > side[0][row]:
            X[row], has[row] = solve(A[row], b[row], reg, ne[row]), 1
    return X, has


def sides(user, item, rel, n_users, n_items):
    """(item side, user side) of a log: rows by (item, user, row) and by (user, item, row)"""
    user, item, rel = np.asarray(user, np.int64), np.asarray(item, np.int64), np.asarray(rel, np.float64)
    out = []
    for grp, key, n in ((item, user, n_items), (user, item, n_users)):
        perm = np.lexsort((np.arange(len(grp)), key, grp))
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(grp, minlength=n), out=off[1:])
        out.append((off, key[perm], rel[perm]))
    return out


def fit(user, item, rel, n_users, n_items, U0, implicit, alpha, reg, iters, store=np.float32):
    """the iteration of section 3.10 from the initial user factors U0; factors are rounded to `store` after every
    solve, as the device stores them.  Returns the list of (U, V) after every iteration."""
    item_side, user_side = sides(user, item, rel, n_users, n_items)
    U, out = np.asarray(U0, dtype=store), []
    for _ in range(iters):
        V = half_step(item_side, U, implicit, alpha, reg)[0].astype(store)
        U = half_step(user_side, V, implicit, alpha, reg)[0].astype(store)
        out.append((U, V))
    return out


def implicit_objective(user, item, rel, U, V, alpha, reg):
    """sum over ALL (u, i) of c_ui (p_ui - x_u . y_i)^2 + reg (sum n_expl(u) |x_u|^2 + sum n_expl(i) |y_i|^2) with
    c_ui = 1 + alpha sum |rho| and p_ui = 1 where the pair has a positive rating -- for a log without duplicated pairs"""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    C, Pm = np.ones((U.shape[0], V.shape[0])), np.zeros((U.shape[0], V.shape[0]))
    nu, ni = np.zeros(U.shape[0]), np.zeros(V.shape[0])
    for u, i, rho in zip(user, item, rel):
        C[u, i] += alpha * abs(rho)
        if rho > 0:
            Pm[u, i] = 1.0
            nu[u] += 1
            ni[i] += 1
    E = Pm - U @ V.T
    return float((C * E * E).sum() + reg * ((nu * (U * U).sum(1)).sum() + (ni * (V * V).sum(1)).sum()))


def dots(X, Y):
    """(fp64 dot, sum of |x_k y_k|) of every pair of rows of X and Y"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return X @ Y.T, np.abs(X) @ np.abs(Y).T
