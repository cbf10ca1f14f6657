"""A numpy-only yardstick of SLIM, written from the normative text of DESIGN.md section 3.15 (not from any
implementation), in a floating-point type of the caller's choice: numpy.float64, or numpy.longdouble.

The problem, per target item j, with nu = n_users, over w >= 0 with w_j = 0:

    F(w) = 1/(2 nu) |x_j - X w|^2 + lambda_ |w|_1 + beta/2 |w|^2
         = (G_jj - 2 w.G[:, j] + w^T G w) / (2 nu) + lambda_ sum(w) + beta/2 sum(w^2),     G = X^T X

which is sklearn's ElasticNet(alpha = beta + lambda_, l1_ratio = lambda_ / alpha, positive=True, fit_intercept=False) on
X with column j zeroed.

The descent (`descend`): from w = 0, q = G[:, j]; a sweep visits i = 0 .. n-1 ascending, i != j: d = G_ii + nu beta; if
d <= 0 the coordinate stays 0; else new = max(0, (q_i + G_ii w_i) - nu lambda_) / d; where new != w_i:
q = q - (new - w_i) G[i, :], w_i = new.  After each full sweep q is recomputed from w (`refresh`): element by element
((G_ej - w_k1 G_k1,e) - w_k2 G_k2,e) - ... over the support k ascending; the certificate is taken from that q; the
column is done at max |v_i| <= tol lambda_ or after max_iter sweeps.  A column with G_jj = 0 is all zeros, no sweep.
A coordinate whose update is zero leaves q unchanged, so `descend` evaluates all remaining coordinates at once and
jumps to the first whose update is not zero: the same iterates as the one-by-one loop (`descend_plain`, kept for the
test that says so).

The certificate (`certificate`): g_i = (-q_i) / nu + beta w_i + lambda_ with q = G[:, j] - G w;
v_i = g_i where w_i > 0, min(g_i, 0) where w_i = 0, v_j = 0.  v is the element of smallest norm of the subdifferential
of Phi = F + (the indicator of K = {w >= 0, w_j = 0}) at w: at w_i = 0 the l1 term and the cone together give the
interval (-inf, g_i], whose smallest element in absolute value is min(g_i, 0); on coordinate j the cone is the whole
line.  w minimises Phi exactly when v = 0.

The two bounds the tests assert (derived, not fitted).  F is beta-strongly convex and K is convex, so the
subdifferential of Phi is beta-strongly monotone: for w1, w2 in K with v1, v2 as above
    beta |w1 - w2|_2^2 <= <v1 - v2, w1 - w2> <= (|v1|_2 + |v2|_2) |w1 - w2|_2,  so  |w1 - w2|_2 <= (|v1|_2 + |v2|_2) / beta.
With beta = 0 convexity alone gives F(w1) - F(w2) <= <v1, w1 - w2> <= |v1|_inf |w1 - w2|_1, which the tests use in the
symmetric form (|v1|_inf + |v2|_inf) |w1 - w2|_1.

Rounding of the device's certificate (`refresh_rounding`).  u = 2^-53.  The device evaluates, in float64 and as written,
q^_i = ((G_ij - w_k1 G_k1,i) - ...) over the s support entries, then g^_i = ((-q^_i) / nu + beta w_i) + lambda_.  Count the
roundings each input passes through: a product w_k G_ki is rounded once and passes at most s subtractions, G_ij passes s
subtractions; the division by nu is one more; the two additions of g are two more.  So everything that comes from q
carries at most s + 4 roundings; beta w_i carries its product and two additions, 3; lambda_ carries the last addition, 1:
    |g^_i - g_i| <= r_i = gamma_{s+4} (|G_ij| + sum_k |G_ik| w_k) / nu + gamma_3 beta w_i + gamma_1 lambda_,
gamma_m = m u / (1 - m u).  (A count that stops at the division, (s + 2) on the first term and 2 on beta w_i + lambda_,
leaves out that the two final additions also round the q term; this one does not.)  v_i is g_i or min(g_i, 0), both
1-Lipschitz in g_i, and whether w_i > 0 is the same on both sides, so |v^_i - v_i| <= r_i and
|max |v^_i| - max |v_i|| <= max r_i.  The host evaluates the same expressions in longdouble from an exact G
(`exact_gram`), which adds the same form with u_L = the longdouble's own unit (`LD_EPS`); `refresh_rounding` takes
u = 2^-53 + LD_EPS to cover both.

Rounding of F (`objective`): evaluated in longdouble as a sum of s^2 + 2 s + 1 products of at most three factors and a
handful of scalings; every term passes fewer than s^2 + 2 s + 8 roundings, so |F^ - F| <= gamma^L_{s^2+2s+8} A with A
the same sum over absolute values, returned beside F."""
import numpy as np

LD = np.longdouble
U = LD(2) ** -53
LD_EPS = LD(np.finfo(LD).eps)


def gamma(m, u=U):
    return LD(m) * u / (1 - LD(m) * u)


def interactions(user, item, relevance, n_users=None, n_items=None, dtype=np.float64):
    """users x items, duplicated (user, item) rows SUMMED, as scipy's csc_matrix sums them"""
    user, item = np.asarray(user, dtype=np.int64), np.asarray(item, dtype=np.int64)
    n_users = int(user.max()) + 1 if n_users is None else n_users
    n_items = int(item.max()) + 1 if n_items is None else n_items
    X = np.zeros((n_users, n_items), dtype=dtype)
    np.add.at(X, (user, item), np.asarray(relevance, dtype=dtype))
    return X


def exact_gram(X):
    """G = X^T X without a rounding, as longdouble: X is scaled by a power of two to integers, multiplied in int64 and
    scaled back; raises where that is not possible (the tests' data are integers or small dyadic fractions)"""
    X = np.asarray(X, dtype=np.float64)
    for k in range(0, 21):
        Xi = X * 2.0 ** k
        if (Xi == np.rint(Xi)).all():
            break
    else:
        raise ValueError("the data are not dyadic fractions with at most 20 binary places")
    Xi = np.rint(Xi)
    top = float(np.abs(Xi).max(initial=0)) ** 2 * X.shape[0]
    if top >= 2.0 ** 62:
        raise ValueError("the integer Gram matrix does not fit int64")
    # every partial sum is an integer below `top`: below 2^53 float64 arithmetic (BLAS) is exact, whatever its order
    Gi = (Xi.T @ Xi).astype(np.int64) if top < 2.0 ** 53 else Xi.astype(np.int64).T @ Xi.astype(np.int64)
    G = Gi.astype(LD) / LD(4) ** k
    assert (G * LD(4) ** k == Gi.astype(LD)).all()
    return G


def refresh(G, j, w):
    """q = G[:, j] - sum over the support, k ascending, of w_k G[k, :], element by element in that order, in G's type"""
    q = G[j].copy()
    for k in np.nonzero(w)[0]:
        q = q - w[k] * G[k]
    return q


def certificate(G, j, w, nu, beta, lambda_):
    """v in longdouble from G (exact, longdouble) and w"""
    G, w = np.asarray(G, dtype=LD), np.asarray(w, dtype=LD)
    q = refresh(G, j, w)
    g = ((-q) / LD(nu) + LD(beta) * w) + LD(lambda_)
    v = np.where(w > 0, g, np.minimum(g, LD(0)))
    v[j] = 0
    return v


def refresh_rounding(G, j, w, nu, beta, lambda_, device=True):
    """r_i of the module text, in longdouble: for the float64 evaluation plus the longdouble one (what separates a
    certificate the device reports from the host's), or with device=False for the longdouble one alone (what separates
    `certificate` from the exact v)"""
    G, w = np.asarray(G, dtype=LD), np.asarray(w, dtype=LD)
    k = np.nonzero(w)[0]
    s = len(k)
    u = U + LD_EPS if device else LD_EPS
    mass = np.abs(G[j]) + np.abs(G[:, k]) @ np.abs(w[k])
    r = gamma(s + 4, u) * mass / LD(nu) + gamma(3, u) * LD(beta) * np.abs(w) + gamma(1, u) * LD(lambda_)
    r[j] = 0
    return r


def objective(G, j, w, nu, beta, lambda_):
    """(F, the bound of its rounding) in longdouble"""
    G, w = np.asarray(G, dtype=LD), np.asarray(w, dtype=LD)
    k = np.nonzero(w)[0]
    s = len(k)
    ws, Gs = w[k], G[np.ix_(k, k)]
    quad = G[j, j] - 2 * np.sum(ws * G[k, j]) + np.sum(ws[:, None] * Gs * ws[None, :])
    F = quad / (2 * LD(nu)) + LD(lambda_) * np.sum(ws) + LD(beta) / 2 * np.sum(ws * ws)
    A = ((np.abs(G[j, j]) + 2 * np.sum(np.abs(ws * G[k, j])) + np.sum(np.abs(ws[:, None] * Gs * ws[None, :]))) / (2 * LD(nu))
         + LD(lambda_) * np.sum(np.abs(ws)) + LD(beta) / 2 * np.sum(ws * ws))
    return F, gamma(s * s + 2 * s + 8, LD_EPS) * A


def _v_up(G, j, w, nu, beta, lambda_):
    """|v_i| of w from above: the longdouble certificate plus its own rounding"""
    return np.abs(certificate(G, j, w, nu, beta, lambda_)) + refresh_rounding(G, j, w, nu, beta, lambda_, device=False)


def distance_and_bound(G, j, w1, w2, nu, beta, lambda_):
    """(|w1 - w2|_2, (|v1|_2 + |v2|_2) / beta) for beta > 0, from the exact G"""
    v1, v2 = _v_up(G, j, w1, nu, beta, lambda_), _v_up(G, j, w2, nu, beta, lambda_)
    diff = np.asarray(w1, dtype=LD) - np.asarray(w2, dtype=LD)
    return np.sqrt(np.sum(diff * diff)), (np.sqrt(np.sum(v1 * v1)) + np.sqrt(np.sum(v2 * v2))) / LD(beta)


def objective_gap_and_bound(G, j, w1, w2, nu, beta, lambda_):
    """(F(w1) - F(w2), (|v1|_inf + |v2|_inf) |w1 - w2|_1 + the rounding of the two evaluations of F), from the exact G"""
    v1, v2 = _v_up(G, j, w1, nu, beta, lambda_), _v_up(G, j, w2, nu, beta, lambda_)
    F1, e1 = objective(G, j, w1, nu, beta, lambda_)
    F2, e2 = objective(G, j, w2, nu, beta, lambda_)
    l1 = np.sum(np.abs(np.asarray(w1, dtype=LD) - np.asarray(w2, dtype=LD)))
    return F1 - F2, (np.max(v1) + np.max(v2)) * l1 + e1 + e2


def _finish(G, j, w, nu, beta, lambda_, dtype):
    q = refresh(G, j, w)
    g = ((-q) / dtype(nu) + dtype(beta) * w) + dtype(lambda_)
    v = np.where(w > 0, g, np.minimum(g, dtype(0)))
    v[j] = 0
    return q, dtype(np.max(np.abs(v)))


def descend(G, j, nu, beta, lambda_, tol=1e-4, max_iter=5000, dtype=np.float64):
    """(w, sweeps, kkt, updates) of the normative descent in `dtype`"""
    G = np.asarray(G, dtype=dtype)
    n = G.shape[0]
    w = np.zeros(n, dtype=dtype)
    if G[j, j] == 0:
        return w, 0, dtype(0), 0
    diag = G.diagonal().copy()
    nb, nl, thr = dtype(nu) * dtype(beta), dtype(nu) * dtype(lambda_), dtype(tol) * dtype(lambda_)
    d = diag + nb
    live = d > 0
    live[j] = False
    safe = np.where(live, d, dtype(1))
    q = G[j].copy()
    sweeps = updates = 0
    while True:
        p = 0
        while p < n:
            r = (q[p:] + diag[p:] * w[p:]) - nl
            new = np.where(live[p:], np.maximum(r, dtype(0)) / safe[p:], w[p:])
            moved = np.nonzero(new != w[p:])[0]
            if not len(moved):
                break
            i = p + int(moved[0])
            q = q - (new[moved[0]] - w[i]) * G[i]
            w[i] = new[moved[0]]
            updates += 1
            p = i + 1
        sweeps += 1
        q, kkt = _finish(G, j, w, nu, beta, lambda_, dtype)
        if kkt <= thr or sweeps >= max_iter:
            return w, sweeps, kkt, updates


def descend_plain(G, j, nu, beta, lambda_, tol=1e-4, max_iter=5000, dtype=np.float64):
    """the same, one coordinate at a time as the text reads"""
    G = np.asarray(G, dtype=dtype)
    n = G.shape[0]
    w = np.zeros(n, dtype=dtype)
    if G[j, j] == 0:
        return w, 0, dtype(0), 0
    nb, nl, thr = dtype(nu) * dtype(beta), dtype(nu) * dtype(lambda_), dtype(tol) * dtype(lambda_)
    q = G[j].copy()
    sweeps = updates = 0
    while True:
        for i in range(n):
            d = G[i, i] + nb
            if i == j or not d > 0:
                continue
            new = max(dtype(0), (q[i] + G[i, i] * w[i]) - nl) / d
            if new != w[i]:
                q = q - (new - w[i]) * G[i]
                w[i] = new
                updates += 1
        sweeps += 1
        q, kkt = _finish(G, j, w, nu, beta, lambda_, dtype)
        if kkt <= thr or sweeps >= max_iter:
            return w, sweeps, kkt, updates


def fit(G, nu, beta, lambda_, tol=1e-4, max_iter=5000, dtype=np.float64, columns=None):
    """(S [n, n] with S[i, j] = w^(j)_i, sweeps, kkt, updates) over `columns` (all by default); other columns are zero"""
    n = G.shape[0]
    S = np.zeros((n, n), dtype=dtype)
    sweeps, kkt, updates = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=dtype), np.zeros(n, dtype=np.int64)
    for j in range(n) if columns is None else columns:
        S[:, j], sweeps[j], kkt[j], updates[j] = descend(G, j, nu, beta, lambda_, tol, max_iter, dtype)
    return S, sweeps, kkt, updates


def random_log(n_users, n_items, p, seed, R, duplicates=0.0, untouched=()):
    """rows (user, item, relevance): RandomState(300 + seed), an entry present with probability p, relevance uniform in
    1..R; a share `duplicates` of the rows is repeated (with a relevance of its own); the items in `untouched` get no
    row; the last user and the last item always get one; the rows are shuffled"""
    rs = np.random.RandomState(300 + seed)
    present = rs.rand(n_users, n_items) < p
    present[:, list(untouched)] = False
    present[n_users - 1, n_items - 1] = True
    user, item = np.nonzero(present)
    if duplicates:
        again = rs.choice(len(user), size=max(1, int(len(user) * duplicates)), replace=False)
        user, item = np.concatenate([user, user[again]]), np.concatenate([item, item[again]])
    order = rs.permutation(len(user))
    user, item = user[order], item[order]
    rel = rs.randint(1, R + 1, size=len(user)).astype(np.float64)
    return user.astype(np.int64), item.astype(np.int64), rel


# the golden logs: name -> (n_users, n_items, p, seed, R, duplicates, untouched)
GOLDEN_LOGS = {"binary": (80, 17, .25, 1, 1, 0.0, ()), "ratings": (150, 33, .15, 2, 5, 0.0, ()),
               "duplicates": (60, 12, .3, 3, 3, 0.2, (7,))}
GOLDEN_PARAMS = [(0.01, 0.01), (0.5, 0.001), (0, 0.01), (1e-3, 0.2)]      # (beta, lambda_)
